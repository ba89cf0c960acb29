"""One validation's evaluation report -- device window scores in, a ScoreReport on the host out, synchronised -- at the table size of
tools/bench_score_device.py: 200 clips x 450 frames x 4 persons x 5 transformations, about 1.76 M windows of 12 frames.

  (a) the host report, the reference's way: eval_utils.score_dataset + eval_utils.score_report (one sklearn call per transformation
      and clip, one roc_curve per transformation)
  (b) eval_utils.score_report_device with a ready plan (csrc/score_frames.hip + csrc/score_report.hip)
  (c) eval_utils.score_dataset_device alone: what the report adds is (b) - (c)

(a), (b) and (c) alternate in one process; median of `--reps` after `--warmup`, with min and max.  Both routes' reports are compared
before any time is printed.  Rows: {"what": ..., "median_ms", "min_ms", "max_ms", "reps"}; then the stages of the report, each
synchronised; the last row carries the verdict: the device route is the report's route if (b) beats (a) by more than (a)'s own
max - min.  Exits non-zero without a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_score_device import row, timed, window_table     # noqa: E402  (the same table, the same protocol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=200); ap.add_argument("--frames", type=int, default=450)
    ap.add_argument("--persons", type=int, default=4); ap.add_argument("--transforms", type=int, default=5)
    ap.add_argument("--seg-len", type=int, default=12); ap.add_argument("--pad-size", type=int, default=-1)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_score_report: needs the GPU", file=sys.stderr)
        return 2
    if a.reps < 5:
        ap.error("--reps: at least 5")
    from coskad_amd import ops
    from coskad_amd.utils import eval_utils as E
    from coskad_amd.utils import score_plan as SP
    trans, meta, frames, gts = window_table(a.clips, a.frames, a.persons, a.transforms, a.seg_len)
    N = trans.shape[0]
    scores = torch.rand(N, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) + 0.05     # float32, as the heads give them
    scores[::101] = 0.0
    kw = dict(pad_size=a.pad_size)
    plan = E.ScorePlan(trans, meta, frames, gts, a.transforms, device="cuda", **kw)
    keys, seg = E.clip_segments(gts)

    def host_report():
        _, per_t, gt = E.score_dataset(scores, trans, meta, frames, gts, a.transforms, **kw)
        return E.score_report(per_t, gt, seg, keys)

    # both routes agree, or no time is printed (their smoothed scores differ in the last bits: test_gpu_score_device.py's tolerance)
    ra, (rb, _, _) = host_report(), E.score_report_device(scores, plan)
    tol = dict(rtol=1e-10, atol=0)
    assert ra.clip_keys == rb.clip_keys and np.array_equal(ra.n_pos, rb.n_pos) and np.array_equal(ra.n_neg, rb.n_neg)
    np.testing.assert_allclose(rb.clip_auc, ra.clip_auc, **tol); np.testing.assert_allclose(rb.clip_auc_final, ra.clip_auc_final, **tol)
    np.testing.assert_allclose(rb.auc_t, ra.auc_t, **tol); np.testing.assert_allclose(rb.auc, ra.auc, **tol)
    for x, y in zip(rb.thresholds_t, ra.thresholds_t):
        assert x.shape == y.shape
        np.testing.assert_allclose(x, y, **tol)
    assert rb.auc == E.score_dataset_device(scores, plan)[0]

    host, dev, base = [], [], []
    for i in range(a.warmup + a.reps):               # (a), (b) and (c) alternate
        ta = timed(host_report, 1, 0)
        tb = timed(lambda: E.score_report_device(scores, plan), 1, 0)
        tc = timed(lambda: E.score_dataset_device(scores, plan), 1, 0)
        if i >= a.warmup:
            host += ta; dev += tb; base += tc
    shape = dict(windows=N, frames_out=plan.F, clips=plan.n_clips, transforms=a.transforms, pad_size=a.pad_size)
    print(json.dumps(row("a: score_dataset + score_report (host)", host, **shape)))
    print(json.dumps(row("b: score_report_device (ready plan)", dev, auc_host=ra.auc, auc_device=rb.auc)))
    print(json.dumps(row("c: score_dataset_device (ready plan)", base)))

    # the parts of (a) and of (b) - (c), each synchronised
    _, per_t_a, gt_a = E.score_dataset(scores, trans, meta, frames, gts, a.transforms, **kw)
    per_t, mean = SP.frame_scores_device(scores, plan)
    tables = plan.report_tables()
    rows = torch.cat([per_t, mean[None]], 0)
    s_all, perm = torch.sort(rows, dim=1, stable=True)
    gt_all = plan.gt_dev[perm]
    cum = torch.cumsum(gt_all == 0, 1)
    stages = [("host: score_report alone", lambda: E.score_report(per_t_a, gt_a, seg, keys)),
              ("report_from_frame_scores", lambda: SP.report_from_frame_scores(per_t, mean, plan.gt_dev, plan.segments_dev,
                                                                                plan.clip_keys, tables=tables)),
              ("sort rows by score", lambda: torch.sort(rows, dim=1, stable=True)),
              ("sort by segment key", lambda: torch.sort(tables[0][perm], dim=1, stable=True)),
              ("auc kernels, whole vector", lambda: ops.score_report_auc(s_all, gt_all, cum, tables[2], tables[3],
                                                                  (plan.F + SP.REPORT_TILE - 1) // SP.REPORT_TILE)),
              ("threshold kernels", lambda: ops.score_report_thresholds(s_all[:a.transforms], cum[:a.transforms]))]
    for name, fn in stages:
        print(json.dumps(row("stage: " + name, timed(fn, a.reps, a.warmup))))
    ma, mb, mc = statistics.median(host), statistics.median(dev), statistics.median(base)
    print(json.dumps({"what": "verdict", "a_over_b": round(ma / mb, 2), "report_adds_ms": round(mb - mc, 3),
                      "a_spread_ms": round(max(host) - min(host), 3),
                      "b_beats_a_by_more_than_a_spread": bool(ma - mb > max(host) - min(host))}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
