"""What the per-joint error map costs (csrc/eval_tail_window.hip's map kernel), same batch, same process, B = 4096 over
T in {8, 12, 24} x V in {17, 25}:

Launch rows {"what": "launch", T, V, Ci, ...}: ops.layer_tail_map against the score-only ops.layer_tail on the same [B, Ci, T, V]
tensors, Ci in {16, 32}.  The map adds B T V 4 bytes of stores to a launch that reads B (Ci + 2) T V 4: 1 / (Ci + 2) of its traffic.
`miss`: the measured surplus exceeds twice that share plus the spread ((max - min) / median) of the score-only samples of the same run.

Wrapper rows {"what": "wrapper", T, V, ...}: LitAutoEncoder.window_error_map against window_scores_from_batch ('rec') on the default
autoencoder (latent 16).

The two routes of a row alternate sample by sample; a sample is `--calls` calls between two device events.  After the warm-up,
`--samples` (>= 20) samples a route: median, min and max in microseconds per call.

    timeout 600 python tools/bench_error_map.py [--batch 4096] [--samples 24] [--calls 20]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = (8, 12, 24)
JOINTS = (17, 25)


def _sample(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls        # microseconds per call


def _alternate(fa, fb, a):
    """-> (samples of fa, samples of fb) in microseconds per call, taken alternately after a warm-up of both"""
    import torch
    for _ in range(a.warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.samples):
        ta.append(_sample(fa, a.calls))
        tb.append(_sample(fb, a.calls))
    return ta, tb


def _stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}


def _row(what, base, new, **keys):
    mb, mn = statistics.median(base), statistics.median(new)
    return dict(keys, what=what, samples=len(base), base=_stats(base), map=_stats(new), ratio=round(mn / mb, 4),
                base_spread=round((max(base) - min(base)) / mb, 4))


def bench_launch(T, V, Ci, a):
    import torch
    from coskad_amd import ops
    B = a.batch
    g = torch.Generator().manual_seed(T * 100 + V + Ci)
    h = torch.randn(B, Ci, T, V, generator=g).cuda()
    x = torch.randn(B, 2, T, V, generator=g).cuda()
    A, Tm = (torch.randn(T, V, V, generator=g) * 0.3).cuda(), (torch.randn(V, T, T, generator=g) * 0.3).cuda()
    wfold, bias = torch.zeros(2 * Ci, 16), torch.zeros(16)
    wfold[:, :2] = torch.randn(2 * Ci, 2, generator=g) / (2 * Ci) ** 0.5
    bias[:2] = torch.randn(2, generator=g) * 0.5
    wfold, bias = wfold.cuda(), bias.cuda()
    slope = torch.full((1,), 0.25).cuda()
    score, score2 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    emap = torch.empty(B, T, V, device="cuda")

    def base():
        ops.layer_tail(h, A, Tm, wfold, bias, 2, in_slope=slope, out_slope=slope, x=x, want_out=False, want_score=True, score=score)

    def with_map():
        ops.layer_tail_map(h, A, Tm, wfold, bias, 2, x, in_slope=slope, out_slope=slope, score=score2, emap=emap)

    tb, tm = _alternate(base, with_map, a)
    assert torch.equal(score, score2), "the map launch's score differs"
    row = _row("launch", tb, tm, T=T, V=V, Ci=Ci, batch=B)
    row["share"] = round(1.0 / (Ci + 2), 4)
    row["miss"] = bool(row["ratio"] - 1.0 > 2 * row["share"] + row["base_spread"])
    row["base_gbps"] = round(B * ((Ci + 2) * T * V + 1) * 4 / (row["base"]["median_us"] * 1e-6) / 1e9, 1)
    return row


def bench_wrapper(T, V, a):
    import torch
    import yaml
    from argparse import Namespace
    from coskad_amd import lit
    from coskad_amd.utils.argparser import init_sub_args
    from coskad_amd.utils.synthetic import synthetic_clips
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_autoencoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(create_experiment_dir=False, dataset_seg_len=T, dataset_batch_size=a.batch)
    joints = lit._joints
    lit._joints = lambda args: V                    # the wrappers read the joint count off the dataset keys (14 / 17 / 18): 25 is set here
    try:
        args, *_ = init_sub_args(Namespace(**cfg))
        torch.manual_seed(0)
        w = lit.LitAutoEncoder(args).cuda()
    finally:
        lit._joints = joints
    w.model.eval()
    w.score_type = 'rec'
    x = synthetic_clips(a.batch, 2, T, V, seed=1).cuda()
    with torch.no_grad():
        assert w.model._tail_layer(x) is not None, "the default autoencoder scores on the tail kernel"

    def base():
        with torch.no_grad():
            return w.window_scores_from_batch(x)

    def with_map():
        return w.window_error_map(x)

    assert torch.equal(base(), with_map()[0]), "window_error_map's rec differs from the window scores"
    tb, tm = _alternate(base, with_map, a)
    return _row("wrapper", tb, tm, T=T, V=V, batch=a.batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert a.samples >= 20, "the median of at least 20 samples"
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    torch.cuda.set_device(0)
    for V in JOINTS:
        for T in WINDOWS:
            for Ci in (16, 32):
                print(json.dumps(bench_launch(T, V, Ci, a)), flush=True)
            print(json.dumps(bench_wrapper(T, V, a)), flush=True)


if __name__ == "__main__":
    main()
