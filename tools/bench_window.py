"""Window-length timing (dataset_seg_len): the space-time mixing kernels at T in {8, 12, 16, 24} x V in {17, 25} and the
default-width one-class step (STS-GCN 2-32-16-32-64, `linear` projector, latent 16, Euclidean head) at B = 4096.

Per (T, V): the mixing forward, its adjoint and the one-pass parameter + input gradient kernel (`gcn_bwd_params_dx`) at C = 32
(rows = B * C), as us and as achieved GB/s on their algorithmic bytes -- the row tensors read and written: 2 for the mix and the
adjoint, 3 (x, dZ in, dX out) for the gradient kernel; tables and partial rows excluded.  The kernels sit below the fp32 MFMA ridge
(<= 12 FLOP / byte at (24, 25)), so they are held to an HBM figure: the T = 12 kernel's GB/s at the same V measured IN THIS RUN,
minus 3 % (twice the +-1.5 % box-to-box spread).  T = 12 runs the tile-image kernels of stsgcn_fwd.hip / stsgcn_bwd.hip, the other
window lengths csrc/gcn_window.hip.  Warm-up first, then the median of >= 3 timed blocks (HIP events; every block printed).

    timeout 600 python tools/bench_window.py [--batch 4096] [--blocks 3] [--steps 10] [--kernels-only]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOWS = (8, 12, 16, 24)
JOINTS = (17, 25)
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


def bench_kernels(T: int, V: int, B: int, C: int, warmup: int, blocks: int, steps: int):
    from coskad_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T * 100 + V)
    x = torch.randn(B, C, T, V, device="cuda", generator=g)
    dZ = torch.randn(B, C, T, V, device="cuda", generator=g)
    A = torch.randn(T, V, V, device="cuda", generator=g) * 0.3
    Tm = torch.randn(V, T, T, device="cuda", generator=g) * 0.3
    dA, dT = torch.empty_like(A), torch.empty_like(Tm)
    tensor_bytes = 4.0 * x.numel()
    res = {}
    for name, fn, n_tensors in (("forward", lambda: ops.gcn(x, A, Tm), 2), ("adjoint", lambda: ops.gcn(dZ, A, Tm, adjoint=True), 2),
                                ("params_dx", lambda: ops.gcn_bwd_params_dx(x, dZ, A, Tm, dA=dA, dT=dT), 3)):
        t = _time_blocks(fn, warmup, blocks, steps)
        med = statistics.median(t)
        res[name] = {"blocks_us": [round(1e3 * v, 2) for v in t], "median_us": round(1e3 * med, 2),
                     "gbps": round(n_tensors * tensor_bytes / (med * 1e-3) / 1e9, 1)}
    return res


def bench_step(T: int, V: int, B: int, warmup: int, blocks: int, steps: int):
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import make_train_step
    from oracle import ref_cpu as R
    m = STSE(2, [32, 16, 32], 64, 16, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0).cuda().train()
    m.c.copy_(torch.linspace(-0.2, 0.2, 16))
    eng = make_train_step(m, lr=1e-4, alpha=1e-6, head='euclidean')
    x = R.synthetic_clips(B, T=T, V=V, seed=1).cuda()
    return type(eng).__name__, [s.kind for s in eng.stack.segs], _time_blocks(lambda: eng.step(x), warmup, blocks, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="mixing kernels only (for a rocprofv3 run)")
    args = ap.parse_args()
    assert args.blocks >= 3
    torch.cuda.set_device(0)
    for V in JOINTS:
        kern = {T: bench_kernels(T, V, args.batch, args.channels, args.warmup, args.blocks, args.steps) for T in WINDOWS}
        for T in WINDOWS:
            row = {"what": "mixing", "T": T, "V": V, "rows": args.batch * args.channels, **kern[T]}
            if T != 12:     # held to the T = 12 kernel at the same V, same run
                row["vs_T12"] = {k: round(kern[T][k]["gbps"] / kern[12][k]["gbps"], 3) for k in kern[T]}
                row["meets_T12_minus_3pct"] = {k: kern[T][k]["gbps"] >= MARGIN * kern[12][k]["gbps"] for k in kern[T]}
            print(json.dumps(row), flush=True)
        if args.kernels_only:
            continue
        for T in WINDOWS:
            cls, kinds, blocks = bench_step(T, V, args.batch, args.warmup, args.blocks, args.steps)
            print(json.dumps({"what": "step", "T": T, "V": V, "batch": args.batch, "engine": cls, "segments": kinds,
                              "blocks_ms": [round(t, 4) for t in blocks], "median_ms": round(statistics.median(blocks), 4)}), flush=True)


if __name__ == "__main__":
    main()
