"""One validation's frame scoring -- device window scores in, an AUC float out, synchronised -- at the order of magnitude of UBnormal's
test split: 200 clips x 450 frames x 4 persons x 5 transformations, about 1.76 M windows of 12 frames.  Window table only: no poses.

  (a) eval_utils.score_dataset as it stands (torch device ops for the keyed aggregation, host smoothing, sklearn)
  (b) eval_utils.score_dataset_device with a ready plan (csrc/score_frames.hip)
  (c) ScorePlan construction alone
  (d) plan.matches alone (what a validation pays on top of (b) to know that the plan is still the table's)

(a) and (b) alternate in one process; median of `--reps` after `--warmup`, with min and max.  Both routes' outputs are compared before any
time is printed.  `--tables cpu` (default) hands the table over as the loaders do, as host tensors; `--tables cuda` as the multi-rank
gather does.  Rows: {"what": ..., "median_ms", "min_ms", "max_ms", "reps"}; the last row carries the ratio (a) / (b).  Exits non-zero
without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window_table(clips, frames, persons, transforms, T, seed=0):
    """(trans [N] int64, meta [N, 4] int64, frames [N, T] int32, gts): every person present throughout, like synthetic.make_dataset"""
    rng = np.random.default_rng(seed)
    starts = np.arange(frames - T + 1)
    cl, pe, st, tr = np.meshgrid(np.arange(clips), np.arange(persons), starts, np.arange(transforms), indexing="ij")
    cl, pe, st, tr = (a.reshape(-1) for a in (cl, pe, st, tr))
    meta = np.stack([cl // 20 + 1, cl % 20 + 1, pe, st], 1).astype(np.int64)
    fr = (st[:, None] + np.arange(1, T + 1)[None]).astype(np.int32)
    gts = {}
    for c in range(clips):
        g = np.zeros(frames, dtype=np.int64)
        a0 = int(rng.integers(20, frames - 80))
        g[a0:a0 + 60] = 1
        gts[(c // 20 + 1, c % 20 + 1)] = g
    return torch.from_numpy(tr.astype(np.int64)), torch.from_numpy(meta), torch.from_numpy(fr), gts


def timed(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def row(what, ms, **extra):
    r = {"what": what, "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
         "reps": len(ms)}
    r.update(extra)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200); ap.add_argument("--frames", type=int, default=450)
    ap.add_argument("--persons", type=int, default=4); ap.add_argument("--transforms", type=int, default=5)
    ap.add_argument("--seg-len", type=int, default=12); ap.add_argument("--pad-size", type=int, default=-1)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tables", choices=["cpu", "cuda"], default="cpu")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_score_device: needs the GPU", file=sys.stderr)
        return 2
    if a.reps < 5:
        ap.error("--reps: at least 5")
    from coskad_amd.utils import eval_utils as E
    trans, meta, frames, gts = window_table(a.clips, a.frames, a.persons, a.transforms, a.seg_len)
    if a.tables == "cuda":
        trans, meta, frames = trans.cuda(), meta.cuda(), frames.cuda()
    N = trans.shape[0]
    scores = torch.rand(N, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) + 0.05     # float32, as the heads give them
    scores[::101] = 0.0
    kw = dict(pad_size=a.pad_size)

    t0 = time.perf_counter()
    plan = E.ScorePlan(trans, meta, frames, gts, a.transforms, device="cuda", **kw)
    torch.cuda.synchronize()
    first_plan_ms = (time.perf_counter() - t0) * 1e3

    # both routes agree, or no time is printed
    auc_a, per_t_a, gt_a = E.score_dataset(scores, trans, meta, frames, gts, a.transforms, **kw)
    auc_b, per_t_b, gt_b = E.score_dataset_device(scores, plan)
    per_t_b = per_t_b.cpu().numpy()
    assert np.array_equal(gt_a, gt_b)
    for t in range(a.transforms):
        np.testing.assert_allclose(per_t_b[t], per_t_a[t], rtol=1e-10, atol=1e-12)
    assert abs(auc_a - auc_b) < 1e-9, (auc_a, auc_b)
    assert plan.matches(trans, meta, frames)

    host, dev = [], []
    for i in range(a.warmup + a.reps):               # (a) and (b) alternate
        ta = timed(lambda: E.score_dataset(scores, trans, meta, frames, gts, a.transforms, **kw), 1, 0)
        tb = timed(lambda: E.score_dataset_device(scores, plan), 1, 0)
        if i >= a.warmup:
            host += ta; dev += tb
    build = timed(lambda: E.ScorePlan(trans, meta, frames, gts, a.transforms, device="cuda", **kw), 5, 0)
    match = timed(lambda: plan.matches(trans, meta, frames), a.reps, a.warmup)
    shape = dict(windows=N, frames_out=plan.F, persons=plan.n_persons, transforms=a.transforms, pad_size=a.pad_size, tables=a.tables)
    print(json.dumps(row("a: score_dataset", host, **shape)))
    print(json.dumps(row("b: score_dataset_device (ready plan)", dev, auc_host=auc_a, auc_device=auc_b)))
    print(json.dumps(row("c: ScorePlan construction", build, first_ms=round(first_plan_ms, 3))))
    print(json.dumps(row("d: plan.matches", match)))
    # the stages of (b) one at a time, each synchronised (so each figure carries one launch + one wait of the host)
    from coskad_amd import ops
    pf = ops.score_person_frames(scores, plan.win_ptr, plan.win_idx)
    raw = ops.score_clip_max(pf, plan.row_ptr, plan.pc_ptr, plan.out_clip, plan.out_frame, plan.n_clips, a.transforms)
    per_t, mean = ops.score_smooth(raw, plan.tiles, plan.taps)
    stages = [("person_frames", lambda: ops.score_person_frames(scores, plan.win_ptr, plan.win_idx)),
              ("pad (pad_size 4)", lambda: ops.score_pad_(pf.clone(), plan.row_ptr, 4, plan.n_max)),
              ("pf.clone() alone", lambda: pf.clone()),
              ("clip_max", lambda: ops.score_clip_max(pf, plan.row_ptr, plan.pc_ptr, plan.out_clip, plan.out_frame, plan.n_clips,
                                                      a.transforms)),
              ("smooth", lambda: ops.score_smooth(raw, plan.tiles, plan.taps)),
              ("auc (sort + cumsum + kernels + copy)", lambda: E.auc_device(mean, plan.gt_dev))]
    for name, fn in stages:
        print(json.dumps(row("stage: " + name, timed(fn, a.reps, a.warmup))))
    ma, mb, md = statistics.median(host), statistics.median(dev), statistics.median(match)
    print(json.dumps({"what": "ratio", "a_over_b": round(ma / mb, 2), "a_over_b_plus_d": round(ma / (mb + md), 2),
                      "b_beats_a_by_more_than_3_percent": bool(mb < ma / 1.03)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
