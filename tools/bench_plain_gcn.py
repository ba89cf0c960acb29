"""Plain-GCN timing: the UBnormal Euclidean model (Learnable_GCN 2-32-16-32-64, `mlp` projector [16] -> 16) at V = 17 and
B in {2048, 4096}:

  (a) the flat step (STSETrainStep on csrc/plain_gcn.hip) against AutogradTrainStep on the same weights, in the same run;
  (b) per layer, the fused forward against the two-GEMM composition and the fused backward (+ the adjacency-gradient reduction)
      against the composed backward (`_PlainGCNLayerFn`), in the same run;
  (c) per layer, the share of max(FLOP / 157.3 TF, bytes / 8 TB/s) on algorithmic FLOP and bytes from the shapes.

Warm-up first, then the median of 3 blocks x 5 steps of HIP-event wall time (every block printed).  A row is a gain when it beats
its yardstick by more than 3 % (twice the +-1.5 % box-to-box spread); everything else is printed as a miss.

    python tools/bench_plain_gcn.py [--batches 2048,4096] [--blocks 3] [--steps 5] [--layers-only] [--static]

Kernel times: `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_plain_gcn.py --layers-only`."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12
MARGIN = 0.03
WIDTHS = [2, 32, 16, 32, 64]


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


def _verdict(new_ms: float, ref_ms: float) -> str:
    return "gain" if new_ms < ref_ms * (1.0 - MARGIN) else "miss"


def _count_calls(fn) -> int:
    """library entry points one call of fn goes through (each is one launch, or one launch + its fixed-order reduction)"""
    from coskad_amd import _lib, ops
    n = [0]
    real = _lib.call

    def counting(*a, **k):
        n[0] += 1
        return real(*a, **k)
    mods = [m for m in sys.modules.values() if getattr(m, "call", None) is real and getattr(m, "__name__", "").startswith("coskad_amd")]
    for m in mods:
        m.call = counting
    try:
        fn()
    finally:
        for m in mods:
            m.call = real
    torch.cuda.synchronize()
    return n[0]


def _count_kernels(fn):
    """GPU kernels of one call of fn as the profiler sees them (torch's own launches included); None where it is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name and "emset" not in e.name)
    except Exception:
        return None


def bench_step(enc: str, B: int, warmup: int, blocks: int, steps: int):
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import make_train_step
    from oracle import ref_cpu as R
    torch.manual_seed(0)
    m = STSE(2, WIDTHS[1:-1], WIDTHS[-1], 16, 12, 17, enc, 'mlp', 'euclidean', 0.0)
    m.c.copy_(torch.linspace(-0.2, 0.2, 16))
    x = R.synthetic_clips(B, seed=1).cuda()
    res = {}
    for name, flat in (("flat", True), ("autograd", False)):
        eng = make_train_step(copy.deepcopy(m).cuda().train(), flat_plain_gcn=flat, lr=1e-4, alpha=1e-6, head='euclidean')
        t = _time_blocks(lambda: eng.step(x), warmup, blocks, steps)
        res[name] = {"engine": type(eng).__name__, "blocks_ms": [round(v, 4) for v in t], "median_ms": round(statistics.median(t), 4),
                     "lib_calls_per_step": _count_calls(lambda: eng.step(x)), "gpu_kernels_per_step": _count_kernels(lambda: eng.step(x))}
    res["verdict"] = _verdict(res["flat"]["median_ms"], res["autograd"]["median_ms"])
    res["speedup"] = round(res["autograd"]["median_ms"] / res["flat"]["median_ms"], 3)
    return res


def bench_layer(Ci: int, Co: int, P: int, B: int, learn: bool, need_dx: bool, warmup: int, blocks: int, steps: int):
    from coskad_amd import ops
    from coskad_amd.models.common.alternative_components import _PlainGCNLayerFn
    from coskad_amd.trainer import _FnCtx
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn(B, Ci, P, device="cuda", generator=g)
    W = (torch.rand(Ci, Co, device="cuda", generator=g) * 2 - 1) / Co ** 0.5
    b = torch.zeros(Co, device="cuda")
    Ap = ops.softmax_rows(torch.rand(P, P, device="cuda", generator=g))
    dO = torch.randn(B, Co, P, device="cuda", generator=g)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    save = learn or Ci <= Co
    O, S = ops.plain_gcn_fwd(X, W, Ap, b, save=save)
    ctx = _FnCtx()
    _PlainGCNLayerFn.forward(ctx, X, W, Ap, b)
    ctx.needs_input_grad = (need_dx, True, learn, True)

    def fused_bwd():
        _, D = ops.plain_gcn_bwd(X, S, O, dO, W, Ap, dW, db, need_dx=need_dx, need_da=learn)
        if learn:
            ops.gemm_rows_outer(D.view(-1, P), (X if Ci <= Co else S).view(-1, P), torch.empty(P, P, device="cuda"))

    t = {"fused_fwd_eval": _time_blocks(lambda: ops.plain_gcn_fwd(X, W, Ap, b), warmup, blocks, steps),
         "fused_fwd_train": _time_blocks(lambda: ops.plain_gcn_fwd(X, W, Ap, b, save=save), warmup, blocks, steps),
         "composed_fwd": _time_blocks(lambda: _PlainGCNLayerFn.forward(_FnCtx(), X, W, Ap, b), warmup, blocks, steps),
         "fused_bwd": _time_blocks(fused_bwd, warmup, blocks, steps),
         "composed_bwd": _time_blocks(lambda: _PlainGCNLayerFn.backward(ctx, dO), warmup, blocks, steps)}
    med = {k: statistics.median(v) for k, v in t.items()}
    Cn = min(Ci, Co)
    f_fwd = B * (2.0 * P * P * Cn + 2.0 * P * Ci * Co)
    by_fwd = 4.0 * B * (Ci + Co) * P
    # backward: dW and the narrow-side gradient (two channel products), the dX mixing, the adjacency gradient
    f_bwd = B * (4.0 * P * Ci * Co + (2.0 * P * P * Cn if (need_dx or Ci > Co) else 0.0) + (2.0 * P * P * Cn if learn else 0.0))
    by_bwd = 4.0 * B * P * (2 * Co + (Cn if Ci <= Co else Ci) + (Ci if need_dx else 0))
    roof = lambda f, by: max(f / PEAK_F32_MFMA, by / PEAK_HBM) * 1e3
    return {"layer": f"{Ci}->{Co}", "branch": "mix first" if Ci <= Co else "channel product first", "need_dx": need_dx, "need_da": learn,
            "blocks_ms": {k: [round(v, 4) for v in vs] for k, vs in t.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
            "fwd_verdict": _verdict(med["fused_fwd_train"], med["composed_fwd"]), "bwd_verdict": _verdict(med["fused_bwd"], med["composed_bwd"]),
            "fwd_speedup": round(med["composed_fwd"] / med["fused_fwd_train"], 3), "bwd_speedup": round(med["composed_bwd"] / med["fused_bwd"], 3),
            "roof_fwd_ms": round(roof(f_fwd, by_fwd), 4), "roof_bwd_ms": round(roof(f_bwd, by_bwd), 4),
            "bound_fwd": "MFMA" if f_fwd / PEAK_F32_MFMA > by_fwd / PEAK_HBM else "HBM",
            "fwd_share_of_roof": round(roof(f_fwd, by_fwd) / med["fused_fwd_eval"], 3),
            "bwd_share_of_roof": round(roof(f_bwd, by_bwd) / med["fused_bwd"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2048,4096")
    ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers-only", action="store_true", help="the per-layer rows only (for a rocprofv3 run)")
    ap.add_argument("--static", action="store_true", help="Static_GCN: the fixed graph, no adjacency gradient")
    args = ap.parse_args()
    assert args.blocks >= 3
    torch.cuda.set_device(0)
    enc = "static_gcn" if args.static else "learnable_gcn"
    P = 12 * args.joints
    for B in (int(v) for v in args.batches.split(",")):
        if not args.layers_only:
            print(json.dumps({"what": "step", "encoder": enc, "batch": B, "joints": args.joints,
                              **bench_step(enc, B, args.warmup, args.blocks, args.steps)}), flush=True)
        for i in range(len(WIDTHS) - 1):
            row = bench_layer(WIDTHS[i], WIDTHS[i + 1], P, B, not args.static, i > 0, args.warmup, args.blocks, args.steps)
            print(json.dumps({"what": "layer", "encoder": enc, "batch": B, **row}), flush=True)


if __name__ == "__main__":
    main()
