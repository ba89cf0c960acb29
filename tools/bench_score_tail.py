"""Scoring of the decoder models with the one-clip tail kernel (csrc/eval_tail_window.hip): the default-width
autoencoder (latent 16) and spherical VAE (latent 8) at B = 4096.

Model rows: {"what": "score", "tree", "model", T, V, "tail", blocks_ms, median_ms}: one eval-mode, no-grad
`window_scores_from_batch` of LitAutoEncoder ('rec') for T in {8, 12, 16, 24} x V in {17, 25}, and of LitVAE at (8, 17) and (24, 25).
The yardstick is the PARENT commit: build it in a second checkout and pass `--parent DIR`; the script then times both trees in the
same session, alternating per (T, V), each in a child process that imports the package from that tree (public wrapper surface
only, so the same file runs there).  `"tail": false` rows -- `engine.EVAL_TAIL = False` of this build -- are the cross-check of the
parent's figure.  A (T, V) stays switched on (ops.LAYER_TAIL_OFF) only if its autoencoder row is more than 3 % faster than the
parent's (twice the +-1.5 % box-to-box spread).

Launch rows (this tree only): {"what": "launch", T, V, Ci, "route", us, gbps, launches}: ops.layer_tail (score only; out + score) on
[B, 32, T, V] against what it replaces on the same tensors -- the eval layer of run_stack (composed at 8 / 16 / 24 frames, the chain
layer at 12), its PReLU and the torch score expression.  GB/s on algorithmic bytes: B (Ci + 2) T V 4 read, 4 B written
(+ 2 T V 4 B with `out`).  `launches`: device kernels of one call, counted by torch.profiler (null where it gives none).

Every child runs under a time limit; the first failure ends the run.  Warm-up first, then the median of >= 3 timed blocks x 10 calls
(HIP events; every block printed).

    timeout 1200 python tools/bench_score_tail.py [--parent ../parent] [--batch 4096] [--blocks 3] [--steps 10] [--models-only]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WINDOWS = (8, 12, 16, 24)
JOINTS = (17, 25)
VAE_ROWS = ((8, 17), (24, 25))
MODELS = {"ae": "euclidean_autoencoder.yaml", "vae": "spherical_vae.yaml"}


def _time_blocks(fn, warmup: int, blocks: int, steps: int):
    import torch
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


def _launches(fn):
    """device kernels of one call of fn, or None where the profiler reports none"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def _wrapper(root, model, T, V, B):
    import torch
    import yaml
    from argparse import Namespace
    from coskad_amd import lit
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(root, "config", "synthetic", MODELS[model])), Loader=yaml.FullLoader)
    cfg.update(create_experiment_dir=False, dataset_seg_len=T, dataset_batch_size=B)
    if V != 17:
        lit._joints = lambda a: V                # the wrappers read the joint count off the dataset keys (14 / 17 / 18): 25 is set here
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(0)
    w = (lit.LitAutoEncoder if model == "ae" else lit.LitVAE)(args).cuda()
    assert (w.model.n_frames, w.model.n_joints) == (T, V), (w.model.n_frames, w.model.n_joints)
    w.model.eval()
    return w


def bench_score(root, tree, model, T, V, B, tail, a):
    import torch
    from coskad_amd import engine
    from oracle import ref_cpu as R
    w = _wrapper(root, model, T, V, B)
    x = R.synthetic_clips(B, 2, T, V, seed=1).cuda()

    def call():
        with torch.no_grad():
            return w.window_scores_from_batch(x)

    if not tail:
        engine.EVAL_TAIL = False
    try:
        t = _time_blocks(call, a.warmup, a.blocks, a.steps)
        n = _launches(call)
    finally:
        if not tail:
            engine.EVAL_TAIL = True
    return {"what": "score", "tree": tree, "model": model, "T": T, "V": V, "batch": B, "tail": tail if tree == "this" else None,
            "blocks_ms": [round(v, 4) for v in t], "median_ms": round(statistics.median(t), 4), "launches": n}


def bench_launch(root, T, V, B, a):
    import torch
    from coskad_amd import engine, ops
    from coskad_amd.models.graph_layers.stsgcn import _PReLUFn, layer_tensors, run_stack
    w = _wrapper(root, "ae", T, V, 8)
    last = w.model.decoder.model[-1]
    L = layer_tensors(last)
    Ci = L.Ci
    g = torch.Generator().manual_seed(2)
    h = torch.randn(B, Ci, T, V, generator=g).cuda()
    x = torch.randn(B, 2, T, V, generator=g).cuda()
    slope = w.model.decoder.model[-2].prelu.weight
    rows = []
    with torch.no_grad():
        wfold, bias = engine.eval_fold(L)

        def tail_score():
            return ops.layer_tail(h, L.A, L.T, wfold, bias, 2, in_slope=slope, out_slope=L.slope, x=x, want_out=False, want_score=True)

        def tail_both():
            return ops.layer_tail(h, L.A, L.T, wfold, bias, 2, in_slope=slope, out_slope=L.slope, x=x, want_out=True, want_score=True)

        def replaced():
            u, s = run_stack(h, [last], w.model.decoder._ws, in_slope=slope)
            xr = u if s is None else _PReLUFn.apply(u, s)
            return ((xr - x) ** 2).reshape(B, -1).mean(-1)

        read = B * (Ci + 2) * T * V * 4
        for route, fn, nbytes in (("tail score", tail_score, read + 4 * B), ("tail out+score", tail_both, read + 4 * B + 2 * T * V * 4 * B),
                                  ("replaced", replaced, read + 4 * B)):
            t = _time_blocks(fn, a.warmup, a.blocks, a.steps)
            med = statistics.median(t)
            rows.append({"what": "launch", "T": T, "V": V, "Ci": Ci, "batch": B, "route": route, "blocks_us": [round(1e3 * v, 2) for v in t],
                         "us": round(1e3 * med, 2), "gbps": round(nbytes / (med * 1e-3) / 1e9, 1), "launches": _launches(fn)})
    return rows


def child(a):
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    torch.cuda.set_device(0)
    T, V = a.row
    from coskad_amd import engine
    has_tail = hasattr(engine, "EVAL_TAIL")
    models = ["ae"] + (["vae"] if (T, V) in VAE_ROWS else [])
    for model in models:
        for tail in ((True, False) if has_tail else (True,)):
            print(json.dumps(bench_score(root, a.tree, model, T, V, a.batch, tail, a)), flush=True)
    if has_tail and not a.models_only:
        for row in bench_launch(root, T, V, a.batch, a):
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: timed alternating with this tree")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models-only", action="store_true")
    ap.add_argument("--limit", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--row", type=lambda s: tuple(int(v) for v in s.split(",")), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="this", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.blocks >= 3
    if a.row is not None:
        return child(a)
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    for V in JOINTS:
        for T in WINDOWS:
            for tree, root in trees:
                cmd = [sys.executable, os.path.abspath(__file__), "--row", f"{T},{V}", "--root", root, "--tree", tree, "--batch",
                       str(a.batch), "--blocks", str(a.blocks), "--steps", str(a.steps), "--warmup", str(a.warmup)]
                cmd += ["--models-only"] if a.models_only else []
                env = dict(os.environ, PYTHONPATH=root)
                try:
                    rc = subprocess.run(cmd, timeout=a.limit, cwd=root, env=env).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(json.dumps({"what": "failed", "tree": tree, "T": T, "V": V, "rc": rc}), flush=True)
                    sys.exit(rc)         # nothing more is started on the GPU after a failure


if __name__ == "__main__":
    main()
