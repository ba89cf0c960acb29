"""The decoder models at the window lengths 8 / 16 / 24 on the flat train step: the default-width autoencoder (latent 16)
and spherical VAE (latent 8, `linear` projector) at B = 4096 for T in {8, 16, 24} x V in {17, 25}, one `training_step` of
LitAutoEncoder / LitVAE with the yaml key `fused_window` left at its default and set to false, and the passes of the few-channel
(4 -> 2) layer and of the decoder's 32 -> 16 / 16 -> 32 layers.

Step rows: {"what": "step", "tree", "model", T, V, fused_window, "route", blocks_ms, median_ms}; route = "flat" (STSAETrainStep) or
"autograd" (module surface + torch.optim.Adam).  The yardstick is the PARENT commit, whose wrappers send every window-length decoder
model to the autograd route: build it in a second checkout and pass `--parent DIR`; the script then times both trees in the same
session, alternating per (T, V), each in a child process that imports the package from that tree.  (The wrappers derive the joint
count from the dataset keys, which know 14 / 17 / 18 joints; for the 25-joint rows the script sets the count itself, in both trees.)  `fused_window: false` of this
build is the cross-check of the parent's figure.  A geometry stays switched on (ops.TRAIN_WINDOW_NARROW_OFF) only if its step is
more than 3 % faster than the parent's (twice the +-1.5 % box-to-box spread).

Layer rows (this tree only): tools/bench_train_window.py's `bench_layer` on (4 -> 2), (32 -> 16) and (16 -> 32).

Every child runs under a time limit; the first failure ends the run.  Warm-up first, then the median of >= 3 timed blocks x 10 steps
(HIP events; every block printed).

    timeout 1200 python tools/bench_ae_window.py [--parent ../parent] [--batch 4096] [--blocks 3] [--steps 10] [--steps-only]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WINDOWS = (8, 16, 24)
JOINTS = (17, 25)
LAYER_SHAPES = ((4, 2), (32, 16), (16, 32))     # the virtual last decoder layer and the decoder's window run
MODELS = (("ae", "euclidean_autoencoder.yaml"), ("vae", "spherical_vae.yaml"))


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


def bench_step(root, tree, model, cfg_name, T, V, B, fused, warmup, blocks, steps):
    import torch
    import yaml
    from argparse import Namespace
    from coskad_amd import lit
    from coskad_amd.utils.argparser import init_sub_args
    from oracle import ref_cpu as R
    cfg = yaml.load(open(os.path.join(root, "config", "synthetic", cfg_name)), Loader=yaml.FullLoader)
    cfg.update(create_experiment_dir=False, dataset_seg_len=T, dataset_batch_size=B)
    if V != 17:
        lit._joints = lambda a: V                # the wrappers read the joint count off the dataset keys (14 / 17 / 18): 25 is set here
    if fused is not None:
        cfg["fused_window"] = fused
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(0)
    wrapper = (lit.LitAutoEncoder if model == "ae" else lit.LitVAE)(args).cuda()
    assert (wrapper.model.n_frames, wrapper.model.n_joints) == (T, V), (wrapper.model.n_frames, wrapper.model.n_joints)
    wrapper.model.train()
    if model == "ae":
        wrapper._make_optimiser('ae', lambda_=wrapper.lambda_)
    else:
        wrapper.setup("fit")
    batch = [R.synthetic_clips(B, 2, T, V, seed=1).cuda(), None, None, None]
    t = _time_blocks(lambda: wrapper.training_step(batch, 1), warmup, blocks, steps)
    return {"what": "step", "tree": tree, "model": model, "T": T, "V": V, "batch": B, "fused_window": fused,
            "route": "flat" if wrapper._flat is not None else "autograd", "blocks_ms": [round(v, 4) for v in t],
            "median_ms": round(statistics.median(t), 4)}


def child(args):
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    torch.cuda.set_device(0)
    T, V = args.row
    import inspect
    from coskad_amd import trainer
    has_flag = "fused_window" in inspect.signature(trainer.STSAETrainStep.__init__).parameters
    for model, cfg_name in MODELS:
        for fused in ((None, False) if has_flag else (None,)):
            print(json.dumps(bench_step(root, args.tree, model, cfg_name, T, V, args.batch, fused, args.warmup, args.blocks, args.steps)),
                  flush=True)
    if has_flag and not args.steps_only:
        sys.path.insert(0, os.path.join(root, "tools"))
        from bench_train_window import bench_layer
        for Ci, Co in LAYER_SHAPES:
            print(json.dumps(bench_layer(T, V, Ci, Co, args.batch, args.warmup, args.blocks, args.steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: timed alternating with this tree")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--row", type=lambda s: tuple(int(v) for v in s.split(",")), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="this", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.blocks >= 3
    if args.row is not None:
        return child(args)
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    for V in JOINTS:
        for T in WINDOWS:
            for tree, root in trees:
                cmd = [sys.executable, os.path.abspath(__file__), "--row", f"{T},{V}", "--root", root, "--tree", tree, "--batch",
                       str(args.batch), "--blocks", str(args.blocks), "--steps", str(args.steps), "--warmup", str(args.warmup)]
                cmd += ["--steps-only"] if args.steps_only else []
                env = dict(os.environ, PYTHONPATH=root)
                try:
                    rc = subprocess.run(cmd, timeout=args.limit, cwd=root, env=env).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(json.dumps({"what": "failed", "tree": tree, "T": T, "V": V, "rc": rc}), flush=True)
                    sys.exit(rc)         # nothing more is started on the GPU after a failure


if __name__ == "__main__":
    main()
