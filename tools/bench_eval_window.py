"""Scoring speed at the window lengths 8 / 16 / 24 (dataset_seg_len): the folded one-clip layer kernel of csrc/eval_layer_clip.hip.

(a) --model: the default-width encoder (STS-GCN 2-32-16-32-64, `linear` projector, latent 16) in eval mode under no_grad, `encode` at
    B = 4096, at (T, V) = (8, 17), (16, 17), (24, 17), (8, 25) (--all-geometries: all six).  Only the public model surface is used, so the
    same file runs on a checkout of the commit before these kernels: THAT time is the yardstick (run both in one session, on one box).
    --composed flips engine.EVAL_WINDOW where it exists: the composed route on this build, a cross-check and not the yardstick.
(b) --kernels: every layer shape 16 / 32 -> 16 / 32 / 64 and every first pair 2 -> 32 -> 16 / 32 / 64 at every (T, V) through
    ops.layer_apply / ops.layer_first_pair_apply, as us and as GB/s on the algorithmic bytes (the input and the output tensor), beside
    the same kernel at T = 12, same V and channels, IN THE SAME RUN.  The yardstick is that T = 12 GB/s minus 3 % (twice the +-1.5 %
    box-to-box spread); misses are printed as misses.

Warm-up first, then the median of >= 3 timed blocks (HIP events; every block printed).

    timeout 600 python tools/bench_eval_window.py --model [--composed] [--batch 4096] [--blocks 3] [--steps 10]
    timeout 600 python tools/bench_eval_window.py --kernels"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODEL_GEOMETRIES = ((8, 17), (16, 17), (24, 17), (8, 25))
ALL_GEOMETRIES = tuple((T, V) for V in (17, 25) for T in (8, 16, 24))
MARGIN = 0.97


def _time_blocks(fn, warmup: int, blocks: int, steps: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def bench_model(T: int, V: int, B: int, warmup: int, blocks: int, steps: int):
    from coskad_amd.models.sts.ae import STSE
    from oracle import ref_cpu as R
    torch.manual_seed(0)
    m = STSE(2, [32, 16, 32], 64, 16, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0).cuda().eval()
    x = R.synthetic_clips(B, T=T, V=V, seed=1).cuda()
    with torch.no_grad():
        t = _time_blocks(lambda: m.encode(x), warmup, blocks, steps)
        z = m.encode(x)
    return t, float(z.double().abs().sum())


def bench_layer(T: int, V: int, Ci: int, Co: int, B: int, warmup: int, blocks: int, steps: int):
    """Ci = 2: the first pair 2 -> 32 -> Co"""
    from coskad_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T * 100 + V)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    A, Tm = rnd(T, V, V) * 0.3, rnd(V, T, T) * 0.3
    x = rnd(B, Ci, T, V)
    slope = torch.full((1,), 0.25, device="cuda")
    if Ci == 2:
        w1, b1, w2, b2 = rnd(4, 32) * 0.5, rnd(32), rnd(64, Co) / 8, rnd(Co)
        fn = lambda: ops.layer_first_pair_apply(x, A, Tm, w1, b1, A, Tm, w2, b2, 32, Co, slope)
    else:
        w, b = rnd(2 * Ci, Co) / (2 * Ci) ** 0.5, rnd(Co)
        out = torch.empty(B, Co, T, V, device="cuda")
        fn = lambda: ops.layer_apply(x, A, Tm, w, b, Co, in_slope=slope, out=out)
    t = _time_blocks(fn, warmup, blocks, steps)
    med = statistics.median(t)
    nbytes = 4.0 * B * (Ci + Co) * T * V
    return {"blocks_us": [round(1e3 * v, 2) for v in t], "median_us": round(1e3 * med, 2), "gbps": round(nbytes / (med * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--composed", action="store_true", help="engine.EVAL_WINDOW = False (where the build has it)")
    ap.add_argument("--all-geometries", action="store_true")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.blocks >= 3 and (args.model or args.kernels)
    torch.cuda.set_device(0)
    from coskad_amd import engine
    has_route = hasattr(engine, "EVAL_WINDOW")
    if args.composed and has_route:
        engine.EVAL_WINDOW = False
    route = "composed" if (args.composed or not has_route) else "window_eval"
    if args.model:
        for T, V in (ALL_GEOMETRIES if args.all_geometries else MODEL_GEOMETRIES):
            t, checksum = bench_model(T, V, args.batch, args.warmup, args.blocks, args.steps)
            print(json.dumps({"what": "encode", "T": T, "V": V, "batch": args.batch, "route": route, "build_has_route": has_route,
                              "blocks_ms": [round(v, 4) for v in t], "median_ms": round(statistics.median(t), 4),
                              "sum_abs_z": round(checksum, 3)}), flush=True)
    if args.kernels:
        from coskad_amd import ops
        for V in (17, 25):
            for Ci, Co in [(2, c) for c in (16, 32, 64)] + [(ci, co) for ci in (16, 32) for co in (16, 32, 64)]:
                base = bench_layer(12, V, Ci, Co, args.batch, args.warmup, args.blocks, args.steps)
                print(json.dumps({"what": "layer", "T": 12, "V": V, "Ci": Ci, "Co": Co, **base}), flush=True)
                for T in (8, 16, 24):
                    ok = ops.layer_first_pair_ok(2, 32, Co, T, V) if Ci == 2 else ops.layer_apply_window_ok(T, V, Ci, Co)
                    if not ok:
                        print(json.dumps({"what": "layer", "T": T, "V": V, "Ci": Ci, "Co": Co, "built": False}), flush=True)
                        continue
                    r = bench_layer(T, V, Ci, Co, args.batch, args.warmup, args.blocks, args.steps)
                    print(json.dumps({"what": "layer", "T": T, "V": V, "Ci": Ci, "Co": Co, **r,
                                      "vs_T12": round(r["gbps"] / base["gbps"], 3),
                                      "meets_T12_minus_3pct": r["gbps"] >= MARGIN * base["gbps"]}), flush=True)


if __name__ == "__main__":
    main()
