"""Wide-latent timing: the default-width one-class step (STS-GCN 2-32-16-32-64, `linear` projector, Euclidean head) at B = 4096 and
latent L in {16, 32, 64, 128, 512}, and the bottleneck forward / backward on their own next to torch (F.prelu + F.linear and its
autograd backward on the same shapes) as a yardstick.  Warm-up first, then the median of >= 3 timed blocks (every block printed);
FLOP and bytes come from the shapes below, the roofs from the MI355X peaks (157.3 TF fp32 MFMA, 8 TB/s HBM).

    python tools/bench_wide_latent.py [--latents 16,32,64,128,512] [--blocks 3] [--steps 10] [--kernels-only]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_wide_latent.py --kernels-only`."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
PEAK_HBM = 8.0e12


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


def bench_step(L: int, B: int, warmup: int, blocks: int, steps: int):
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import make_train_step
    from oracle import ref_cpu as R
    m = STSE(2, [32, 16, 32], 64, L, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0).cuda().train()
    m.c.copy_(torch.linspace(-0.2, 0.2, L))
    eng = make_train_step(m, lr=1e-4, alpha=1e-6, head='euclidean')
    x = R.synthetic_clips(B, seed=1).cuda()
    return type(eng).__name__, _time_blocks(lambda: eng.step(x), warmup, blocks, steps)


def bench_bottleneck(L: int, B: int, K: int, warmup: int, blocks: int, steps: int):
    from coskad_amd import engine, ops
    g = torch.Generator(device="cuda").manual_seed(0)
    U = torch.randn(B, K, device="cuda", generator=g)
    W = torch.randn(L, K, device="cuda", generator=g) / K ** 0.5
    b = torch.zeros(L, device="cuda")
    a = torch.tensor([0.25], device="cuda")
    dz = torch.randn(B, L, device="cuda", generator=g)
    ws = engine.Workspace()
    dW, db, da = torch.empty_like(W), torch.empty_like(b), torch.empty_like(a)
    dU = torch.empty_like(U)
    wsb = torch.empty(ops.btlnk_bwd_ws_bytes(B, K, L), dtype=torch.uint8, device="cuda")
    res = {
        "hip_fwd": _time_blocks(lambda: ops.btlnk_fwd(U, W, b, a, ws=ws), warmup, blocks, steps),
        "hip_bwd": _time_blocks(lambda: ops.btlnk_bwd(U, W, dz, a, dW, db, da, wsb, dU=dU), warmup, blocks, steps),
    }
    Ut, Wt, bt, at = (t.clone().requires_grad_(True) for t in (U, W, b, a))
    res["torch_fwd"] = _time_blocks(lambda: torch.nn.functional.linear(torch.nn.functional.prelu(U, a), W, b), warmup, blocks, steps)

    def torch_bwd():
        z = torch.nn.functional.linear(torch.nn.functional.prelu(Ut, at), Wt, bt)
        torch.autograd.grad(z, [Ut, Wt, bt, at], dz)
    res["torch_fwd_bwd"] = _time_blocks(torch_bwd, warmup, blocks, steps)
    flop = 2.0 * B * K * L
    by_fwd = 4.0 * (B * K + L * K + B * L)
    by_bwd = 4.0 * (2 * B * K + 2 * L * K + B * L)     # U read, dU written, W read, dW written (partials excluded)
    roof = lambda f, by: max(f / PEAK_F32_MFMA, by / PEAK_HBM) * 1e3   # ms
    info = {"flop_per_product": flop, "bytes_fwd": by_fwd, "bytes_bwd": by_bwd,
            "roof_fwd_ms": roof(flop, by_fwd), "roof_bwd_ms": roof(2 * flop, by_bwd),
            "bound_fwd": "MFMA" if flop / PEAK_F32_MFMA > by_fwd / PEAK_HBM else "HBM",
            "bound_bwd": "MFMA" if 2 * flop / PEAK_F32_MFMA > by_bwd / PEAK_HBM else "HBM"}
    return res, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latents", default="16,32,64,128,512")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="bottleneck kernels only (for a rocprofv3 run)")
    args = ap.parse_args()
    assert args.blocks >= 3
    torch.cuda.set_device(0)
    K = 64 * 12 * 17
    for L in (int(v) for v in args.latents.split(",")):
        if not args.kernels_only:
            cls, blocks = bench_step(L, args.batch, args.warmup, args.blocks, args.steps)
            print(json.dumps({"what": "step", "latent": L, "batch": args.batch, "engine": cls,
                              "blocks_ms": [round(t, 4) for t in blocks], "median_ms": round(statistics.median(blocks), 4)}), flush=True)
        if L > 16:
            res, info = bench_bottleneck(L, args.batch, K, args.warmup, args.blocks, args.steps)
            med = {k: statistics.median(v) for k, v in res.items()}
            print(json.dumps({"what": "bottleneck", "latent": L, "batch": args.batch, "K": K,
                              "blocks_ms": {k: [round(t, 4) for t in v] for k, v in res.items()},
                              "median_ms": {k: round(v, 4) for k, v in med.items()},
                              "fwd_share_of_roof": round(info["roof_fwd_ms"] / med["hip_fwd"], 3),
                              "bwd_share_of_roof": round(info["roof_bwd_ms"] / med["hip_bwd"], 3), **info}), flush=True)


if __name__ == "__main__":
    main()
