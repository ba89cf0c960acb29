"""Attribution of the one-class encoder (csrc/eval_layer_adj.hip, coskad_amd/attribution.py) at B = 4096, default widths
2-32-16-32-64, latent 16, T in {8, 12, 24} x V in {17, 25}.

Layer rows: {"what": "layer", T, V, Ci, Co, "adjoint_us", "forward_us", "ratio", blocks}: ops.layer_input_grad of the layer against
ops.layer_apply of the same layer on the same tensors in the same process, ALTERNATING by block (adjoint block, forward block, ...).  The
forward kernel moves about the same bytes and MFMA work: it is the yardstick the ratio is reported against.  (The 2 -> 32 layer has no
one-launch forward at 8 / 24 frames: `forward_us` is null there.)

Model rows: {"what": "model", T, V, "attribution_ms", "scores_ms", "ratio", blocks}: LitEncoder.window_attribution(x) against
window_scores(model(x)) of the same batch, alternating by block.

Warm-up first, then the median of >= 3 timed blocks x 10 calls (HIP events; every block printed).  No time is a pass condition.

    timeout 600 python tools/bench_attribution.py [--batch 4096] [--blocks 3] [--steps 10]"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

WINDOWS = (8, 12, 24)
JOINTS = (17, 25)


def _block(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def _alternate(fns, a):
    """[[block times of fns[0]], [.. of fns[1]]] in ms: warm-up of every one, then blocks in turn"""
    import torch
    for fn in fns:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(a.blocks):
        for k, fn in enumerate(fns):
            out[k].append(_block(fn, a.steps))
    return out


def _wrapper(T, V):
    import torch
    import yaml
    from argparse import Namespace
    from coskad_amd import lit
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(create_experiment_dir=False, dataset_seg_len=T)
    joints = lit._joints
    lit._joints = lambda a: V                    # the wrappers read the joint count off the dataset keys (14 / 17 / 18): 25 is set here
    try:
        args, *_ = init_sub_args(Namespace(**cfg))
        torch.manual_seed(0)
        w = lit.LitEncoder(args).cuda()
    finally:
        lit._joints = joints
    assert (w.model.n_frames, w.model.n_joints) == (T, V)
    w.model.eval()
    return w


def bench(T, V, a):
    import torch
    from coskad_amd import attribution, ops
    from coskad_amd.models.graph_layers.stsgcn import layer_tensors
    from oracle import ref_cpu as R
    B = a.batch
    w = _wrapper(T, V)
    x = R.synthetic_clips(B, 2, T, V, seed=1).cuda()
    with torch.no_grad():
        layers = [layer_tensors(m) for m in w.model.encoder.model]
        us, folds = attribution.eval_preactivations(x, layers)
        g = torch.Generator().manual_seed(2)
        for i, L in enumerate(layers):
            h, slope = (us[i - 1], layers[i - 1].slope) if i else (x, None)
            dU = torch.randn(B, L.Co, T, V, generator=g).cuda()
            out_g, out_f = torch.empty_like(h), torch.empty_like(dU)
            wfold, bias = folds[i]
            fns = [lambda: ops.layer_input_grad(dU, h, L.A, L.T, wfold, L.Co, in_slope=slope, out=out_g)]
            one_launch = i > 0 or T == 12
            if one_launch:
                fns.append(lambda: ops.layer_apply(h, L.A, L.T, wfold, bias, L.Co, in_slope=slope, out=out_f))
            t = _alternate(fns, a)
            adj = statistics.median(t[0])
            fwd = statistics.median(t[1]) if one_launch else None
            print(json.dumps({"what": "layer", "T": T, "V": V, "Ci": L.Ci, "Co": L.Co, "batch": B,
                              "adjoint_us": round(1e3 * adj, 2), "forward_us": None if fwd is None else round(1e3 * fwd, 2),
                              "ratio": None if fwd is None else round(adj / fwd, 3),
                              "adjoint_blocks_us": [round(1e3 * v, 2) for v in t[0]],
                              "forward_blocks_us": None if fwd is None else [round(1e3 * v, 2) for v in t[1]]}), flush=True)

        def scores():
            return w.window_scores(w.model(x))

        t = _alternate([lambda: w.window_attribution(x), scores], a)
        att, sc = statistics.median(t[0]), statistics.median(t[1])
        print(json.dumps({"what": "model", "T": T, "V": V, "batch": B, "attribution_ms": round(att, 4), "scores_ms": round(sc, 4),
                          "ratio": round(att / sc, 2), "attribution_blocks_ms": [round(v, 4) for v in t[0]],
                          "scores_blocks_ms": [round(v, 4) for v in t[1]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert a.blocks >= 3
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attribution: needs the GPU (a CPU run measures nothing)")
    torch.cuda.set_device(0)
    for V in JOINTS:
        for T in WINDOWS:
            bench(T, V, a)


if __name__ == "__main__":
    main()
