"""The decoder models at latents beyond 16 on the flat train step: default widths, V = 17, T = 12, B = 4096.

Step rows: one `training_step` of LitAutoEncoder / LitVAE (`linear` projector) at latent_dim in {32, 64, 128, 512} with the yaml key
`flat_wide_latent` left at its default and set to false: {"what": "step", "tree", "model", "L", "flat_wide_latent", "route",
blocks_ms, median_ms}; route = "flat" (STSAETrainStep) or "autograd" (module surface + torch.optim.Adam).  The yardstick is the PARENT
commit, whose wrappers send every such model to the autograd route: build it in a second checkout and pass `--parent DIR`; both trees
are then timed in the same session, alternating per latent, each in a child process that imports the package from that tree.
`flat_wide_latent: false` of this build is the cross-check of the parent's figure.  A latent stays switched on only if its step is
more than 3 % faster than the parent's (twice the +-1.5 % box-to-box spread); otherwise it goes into ops.AE_WIDE_OFF.

Kernel rows (this tree, one process, the two sides alternating per block): rev_btlnk's forward and its backward (dz and dW / db share
one entry point and are timed together) on csrc/rev_btlnk_wide.hip against the ops fallback they replace (the strided GEMM + cat +
copies), with the roof max(2 B N L / 157.3 TF, bytes / 8 TB/s) per product; and the three launches of the PowerSpherical head at
L = 16 (csrc/vae_head.hip, a thread per clip) against L in {32, 512} (a wave per clip), for the record.

Every child runs under a time limit; the first failure ends the run.  Warm-up first, then the median of >= 3 timed blocks x 5 steps
(HIP events; every block printed).

    timeout 1200 python tools/bench_ae_wide_latent.py [--parent ../parent] [--batch 4096] [--blocks 3] [--steps 5] [--only step|kernel]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

LATENTS = (32, 64, 128, 512)
HEAD_LATENTS = (16, 32, 512)
MODELS = (("ae", "euclidean_autoencoder.yaml"), ("vae", "spherical_vae.yaml"))
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8e12          # fp32 MFMA, HBM


def _block(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def _time_blocks(fn, warmup, blocks, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [_block(fn, steps) for _ in range(blocks)]


def _time_alternating(fns, warmup, blocks, steps):
    """-> one list of block times per function, the functions taking turns block by block"""
    import torch
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(blocks):
        for i, fn in enumerate(fns):
            out[i].append(_block(fn, steps))
    return out


def _row(t):
    return {"blocks_ms": [round(v, 4) for v in t], "median_ms": round(statistics.median(t), 4)}


def bench_step(root, tree, model, cfg_name, L, B, wide, warmup, blocks, steps):
    import torch
    import yaml
    from argparse import Namespace
    from coskad_amd import lit
    from coskad_amd.utils.argparser import init_sub_args
    from oracle import ref_cpu as R
    cfg = yaml.load(open(os.path.join(root, "config", "synthetic", cfg_name)), Loader=yaml.FullLoader)
    cfg.update(create_experiment_dir=False, dataset_batch_size=B, latent_dim=L)
    if model == "vae":
        cfg["projector"] = "linear"
    if wide is not None:
        cfg["flat_wide_latent"] = wide
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(0)
    wrapper = (lit.LitAutoEncoder if model == "ae" else lit.LitVAE)(args).cuda()
    assert wrapper.model.latent_dim == L and (wrapper.model.n_frames, wrapper.model.n_joints) == (12, 17)
    wrapper.model.train()
    if model == "ae":
        wrapper._make_optimiser('ae', lambda_=wrapper.lambda_)
    else:
        wrapper.setup("fit")
    batch = [R.synthetic_clips(B, 2, 12, 17, seed=1).cuda(), None, None, None]
    t = _time_blocks(lambda: wrapper.training_step(batch, 1), warmup, blocks, steps)
    return dict({"what": "step", "tree": tree, "model": model, "L": L, "batch": B, "flat_wide_latent": wide,
                 "route": "flat" if wrapper._flat is not None else "autograd"}, **_row(t))


def bench_rev(L, B, N, warmup, blocks, steps):
    """rev_btlnk's forward and backward: the wide kernels and the fallback they replace, alternating"""
    import torch
    from coskad_amd import ops
    g = torch.Generator().manual_seed(L)
    z = torch.randn(B, L, generator=g).cuda()
    W = (torch.randn(N, L, generator=g) / L ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    dH = torch.randn(B, N, generator=g).cuda()
    dW, db = torch.empty_like(W), torch.empty_like(b)
    off = {'fwd': frozenset({L}), 'bwd': frozenset({L})}
    on = {'fwd': frozenset(), 'bwd': frozenset()}

    def run(table, fn):
        def f():
            ops.REV_WIDE_FALLBACK = table
            fn()
        return f
    fwd = lambda: ops.rev_btlnk_fwd(z, W, b)
    bwd = lambda: ops.rev_btlnk_bwd(dH, z, W, dW, db)
    rows = []
    flops = 2.0 * B * N * L
    big, zb, wb = 4.0 * B * N, 4.0 * B * L, 4.0 * N * L
    one = max(flops / PEAK_FLOPS, (big + zb + wb) / PEAK_BYTES)       # a product: the B x N tensor once, z and W once
    roofs = {"fwd": one, "bwd": 2 * one}                              # the backward is two products (dz; dW with db)
    for name, fn in (("fwd", fwd), ("bwd", bwd)):
        wide_t, fall_t = _time_alternating([run(on, fn), run(off, fn)], warmup, blocks, steps)
        rows.append(dict({"what": "rev_btlnk", "product": name, "side": "wide", "L": L, "B": B, "N": N,
                          "roof_ms": round(roofs[name] * 1e3, 4)}, **_row(wide_t)))
        rows.append(dict({"what": "rev_btlnk", "product": name, "side": "fallback", "L": L, "B": B, "N": N,
                          "roof_ms": round(roofs[name] * 1e3, 4)}, **_row(fall_t)))
    ops.REV_WIDE_FALLBACK = on
    return rows


def bench_ps_head(L, B, warmup, blocks, steps):
    """the three launches of the PowerSpherical head (prep, sample, bwd) on given draws"""
    import torch
    from coskad_amd import ops
    g = torch.Generator().manual_seed(L)
    H2 = torch.randn(B, L + 1, generator=g).cuda()
    dz = torch.randn(B, L, generator=g).cuda()
    _, _, _, saved = ops.ps_head_forward(H2[:, :L], H2[:, L:L + 1])
    mean_raw, var_raw, mu, kappa, conc, total, x, eps = saved
    gr = ops.dirichlet_grad(x, conc, total.unsqueeze(-1).expand(B, 2).contiguous(), f64=True)
    zs, kl, ik, dH2 = torch.empty(B, L, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty_like(H2)
    st = ops._stream()

    def three():
        ops.call("coskad_ps_head_prep_f32", mean_raw, L + 1, var_raw, L + 1, mu, kappa, conc, total, B, L, st)
        ops.call("coskad_ps_head_sample_f32", x, eps, mu, kappa, zs, kl, ik, B, L, st)
        ops.call("coskad_ps_head_bwd_f32", dz, x, gr, eps, mu, kappa, mean_raw, L + 1, var_raw, L + 1, 0.3 / B, 0.2 / B, dH2[:, :L],
                 L + 1, dH2[:, L:L + 1], L + 1, B, L, st)
    return dict({"what": "ps_head", "L": L, "B": B, "kernels": "vae_head.hip PerThread" if L <= 16 else "vae_head.hip PerWave"},
                **_row(_time_blocks(three, warmup, blocks, steps)))


def child(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    torch.cuda.set_device(0)
    if args.row == "kernel":
        for L in LATENTS:
            for r in bench_rev(L, args.batch, 64 * 12 * 17, args.warmup, args.blocks, args.steps):
                print(json.dumps(r), flush=True)
        for L in HEAD_LATENTS:
            print(json.dumps(bench_ps_head(L, args.batch, args.warmup, args.blocks, args.steps)), flush=True)
        return
    L = int(args.row)
    for model, cfg_name in MODELS:
        for wide in ((None, False) if args.tree == "this" else (None,)):
            print(json.dumps(bench_step(root, args.tree, model, cfg_name, L, args.batch, wide, args.warmup, args.blocks, args.steps)),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: timed alternating with this tree")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("step", "kernel"), default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--row", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="this", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.blocks >= 3
    if args.row is not None:
        return child(args)
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    jobs = []
    if args.only != "kernel":
        jobs += [(str(L), tree, root) for L in LATENTS for tree, root in trees]
    if args.only != "step":
        jobs.append(("kernel", "this", ROOT))
    for row, tree, root in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--root", root, "--tree", tree, "--batch", str(args.batch),
               "--blocks", str(args.blocks), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        env = dict(os.environ, PYTHONPATH=root)
        try:
            rc = subprocess.run(cmd, timeout=args.limit, cwd=root, env=env).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps({"what": "failed", "tree": tree, "row": row, "rc": rc}), flush=True)
            sys.exit(rc)         # nothing more is started on the GPU after a failure


if __name__ == "__main__":
    main()
