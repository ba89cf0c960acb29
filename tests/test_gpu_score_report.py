"""The evaluation report on the device (csrc/score_report.hip through ops.score_report_auc / score_report_thresholds and
score_plan.report_from_frame_scores / score_report_device) against scikit-learn and the host route eval_utils.score_report: crafted frame
scores whose clip lengths sit at every edge of the tiling, rows whose ROC thresholds are the special cases, the whole route from window
scores, LitEncoder with the `eval_report` key, and eval_COSKAD.py --report."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml
from sklearn.metrics import roc_auc_score

from coskad_amd import ops
from coskad_amd.utils import eval_utils as E
from coskad_amd.utils import score_plan as SP
from coskad_amd.utils.synthetic import batches, make_dataset
from test_gpu_score_device import _args, _mixed_case
from test_score_report_host import (CLIP_NAMES, UNDEFINED, check_crafted_fixture, crafted_report_case, find_threshold_rows,
                                    sklearn_clip_auc)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_memo = {}


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def _crafted():
    """(fixture, the device report, a second run of it): computed once, shared, left unchanged"""
    if "crafted" not in _memo:
        per_t, gt, seg, keys = crafted_report_case()
        check_crafted_fixture(per_t, gt, seg)                  # on the CPU, by scikit-learn, before anything runs on the GPU
        mean = np.mean(per_t, 0)
        dev = (_dev(per_t, torch.float64), _dev(mean, torch.float64), _dev(gt != 0, torch.int32), _dev(seg, torch.int32))
        reps = [SP.report_from_frame_scores(*dev, keys, segments=seg) for _ in range(2)]
        _memo["crafted"] = ((per_t, mean, gt, seg, keys), dev, reps)
    return _memo["crafted"]


def test_clip_aucs_of_the_crafted_fixture():
    (per_t, mean, gt, seg, keys), _, (rep, _) = _crafted()
    nt = per_t.shape[0]
    assert rep.clip_auc.shape == (nt, 8) and rep.clip_keys == keys
    for t in range(nt + 1):
        row, got = (per_t[t], rep.clip_auc[t]) if t < nt else (mean, rep.clip_auc_final)
        assert {CLIP_NAMES[i] for i in np.nonzero(np.isnan(got))[0]} == UNDEFINED, got
        want = np.array([sklearn_clip_auc(gt[a:b], row[a:b]) for a, b in seg.tolist()])
        ok = ~np.isnan(want)
        print(t, got, want)
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)
        assert got[1] == 0.5 and got[3] == 0.5
    np.testing.assert_array_equal(rep.n_pos, [int(gt[a:b].sum()) for a, b in seg.tolist()])
    np.testing.assert_array_equal(rep.n_neg, [int((gt[a:b] == 0).sum()) for a, b in seg.tolist()])
    np.testing.assert_array_equal(rep.segments, seg)
    np.testing.assert_array_equal(rep.frame_scores, mean)
    for t in range(nt):
        np.testing.assert_array_equal(rep.clip_auc_mean_t[t], np.nanmean(rep.clip_auc[t]))


def test_row_aucs_and_the_final_auc():
    (per_t, mean, gt, seg, keys), (per_t_d, mean_d, gt_d, seg_d), (rep, _) = _crafted()
    np.testing.assert_allclose(rep.auc_t, [roc_auc_score(gt, r) for r in per_t], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rep.auc, roc_auc_score(gt, mean), rtol=1e-12, atol=0)
    assert rep.auc == SP.auc_device(mean_d, gt_d) and isinstance(rep.auc, float)     # today's statistic and quotient, to the bit


def test_thresholds_match_roc_curve():
    (per_t, mean, gt, seg, keys), _, (rep, _) = _crafted()
    for t in range(per_t.shape[0]):
        np.testing.assert_array_equal(rep.thresholds_t[t], E.roc_crossing_thresholds(gt, per_t[t]))
    rows, y = find_threshold_rows()                            # inf first; a point on the line; drop_intermediate matters
    s, perm = torch.sort(_dev(rows, torch.float64), dim=1, stable=True)
    cum = torch.cumsum(_dev(y != 0, torch.int32)[perm] == 0, 1)
    out = ops.score_report_thresholds(s, cum).cpu().numpy()
    want = [E.roc_crossing_thresholds(y, r) for r in rows]
    assert want[0].tolist() == [np.inf, 0.9] and len(want[1]) == 2
    for t in range(3):
        print(t, out[t], want[t])
        assert int(out[t, 0]) == len(want[t])
        np.testing.assert_array_equal(out[t, 1:1 + len(want[t])], want[t])
    # ... and the same rows through the report, one segment, 48 frames: less than one tile
    rep2 = SP.report_from_frame_scores(_dev(rows, torch.float64), _dev(rows.mean(0), torch.float64), _dev(y != 0, torch.int32),
                                       _dev([[0, 48]], torch.int32), [(1, 1)])
    for t in range(3):
        np.testing.assert_array_equal(rep2.thresholds_t[t], want[t])
        np.testing.assert_allclose(rep2.clip_auc[t, 0], roc_auc_score(y, rows[t]), rtol=1e-12, atol=0)
        assert rep2.clip_auc[t, 0] == rep2.auc_t[t]            # one segment over the whole vector: the same integers, the same quotient


def test_random_rows_against_the_host_thresholds():
    """200 short rows with ties, all in one launch: the rule for the dropped points and the crossing, case by case"""
    rng = np.random.default_rng(7)
    y = np.zeros(40, dtype=np.int64)
    y[rng.permutation(40)[:17]] = 1
    rows = np.stack([np.round(rng.random(40) + 0.25 * y, 1 + (i % 3)) for i in range(200)], 0)
    s, perm = torch.sort(_dev(rows, torch.float64), dim=1, stable=True)
    cum = torch.cumsum(_dev(y != 0, torch.int32)[perm] == 0, 1)
    out = ops.score_report_thresholds(s, cum).cpu().numpy()
    for t in range(200):
        want = E.roc_crossing_thresholds(y, rows[t])
        assert int(out[t, 0]) == len(want), (t, out[t], want)
        np.testing.assert_array_equal(out[t, 1:1 + len(want)], want, err_msg=str(t))


def test_two_reports_are_bitwise_equal():
    _, _, (a, b) = _crafted()
    assert a.auc == b.auc
    for name in ("auc_t", "clip_auc", "clip_auc_final", "clip_auc_mean_t", "n_pos", "n_neg", "frame_scores"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    for x, y in zip(a.thresholds_t, b.thresholds_t):
        np.testing.assert_array_equal(x, y)


def test_tables_from_device_segments_match_the_plans():
    (per_t, mean, gt, seg, keys), (per_t_d, mean_d, gt_d, seg_d), (rep, _) = _crafted()
    host = SP.report_tables(seg, per_t.shape[1], "cuda")
    for a, b in zip(host, SP.report_tables(seg_d, per_t.shape[1])):
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)
    rep3 = SP.report_from_frame_scores(per_t_d, mean_d, gt_d, seg_d, keys, tables=host)
    np.testing.assert_array_equal(rep3.clip_auc, rep.clip_auc)


def test_a_segment_outside_the_vector_is_refused():
    (per_t, mean, gt, seg, keys), (per_t_d, mean_d, gt_d, seg_d), _ = _crafted()
    bad = seg.copy()
    bad[6, 1] += 5; bad[7] += 5                                # G would end 5 frames past F
    with pytest.raises(ValueError, match="segments"):          # judged on the host where the host knows them
        SP.report_from_frame_scores(per_t_d, mean_d, gt_d, _dev(bad, torch.int32), keys, segments=bad)
    with pytest.raises(ValueError, match=r"segment 6 .* does not lie in"):        # ... and by the kernel, which reads nothing there
        SP.report_from_frame_scores(per_t_d, mean_d, gt_d, _dev(bad, torch.int32), keys)


def test_a_single_class_vector_raises_as_the_auc_does():
    s = torch.rand(2, 300, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="Only one class"):
        SP.report_from_frame_scores(s, s.mean(0), torch.ones(300, dtype=torch.int32, device="cuda"), _dev([[0, 300]], torch.int32),
                                    [(1, 1)])


# ---- from window scores ------------------------------------------------------------------------------------------------------------

def _end_to_end():
    if "e2e" not in _memo:
        (s, trans, meta, frames, gts), kw = _mixed_case()      # 72- and 300-frame clips, pad 6, a 7-frame and a random mask
        plan = E.ScorePlan(trans, meta, frames, gts, device="cuda", **kw)
        rep, per_t_dev, gt = E.score_report_device(s.cuda(), plan)
        auc_host, per_t, gt_host = E.score_dataset(s, trans, meta, frames, gts, **kw)
        keys, seg = E.clip_segments(gts, kw["hr_masks"])
        _memo["e2e"] = (s, plan, rep, per_t_dev, gt, E.score_report(per_t, gt_host, seg, keys), auc_host, (keys, seg))
    return _memo["e2e"]


def test_route_from_window_scores_matches_the_host_report():
    s, plan, rep, per_t_dev, gt, host, auc_host, (keys, seg) = _end_to_end()
    assert keys == plan.clip_keys == rep.clip_keys and np.array_equal(seg, plan.segments) and np.array_equal(seg, rep.segments)
    assert plan.segments_dev.dtype == torch.int32 and plan.segments_dev.cpu().tolist() == seg.tolist()
    tol = dict(rtol=1e-10, atol=0)
    np.testing.assert_array_equal(np.isnan(rep.clip_auc), np.isnan(host.clip_auc))
    np.testing.assert_array_equal(np.isnan(rep.clip_auc_final), np.isnan(host.clip_auc_final))
    assert (~np.isnan(host.clip_auc)).sum() >= 4
    np.testing.assert_allclose(rep.clip_auc, host.clip_auc, **tol)
    np.testing.assert_allclose(rep.clip_auc_final, host.clip_auc_final, **tol)
    np.testing.assert_allclose(rep.clip_auc_mean_t, host.clip_auc_mean_t, **tol)
    np.testing.assert_allclose(rep.auc_t, host.auc_t, **tol)
    np.testing.assert_allclose(rep.auc, host.auc, **tol)
    np.testing.assert_array_equal(rep.n_pos, host.n_pos); np.testing.assert_array_equal(rep.n_neg, host.n_neg)
    for a, b in zip(rep.thresholds_t, host.thresholds_t):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, **tol)
    np.testing.assert_allclose(rep.frame_scores, host.frame_scores, rtol=1e-10, atol=1e-12)
    # the report's AUC is score_dataset_device's, to the bit, and so are the frame scores next to it
    auc, per_t2, _ = E.score_dataset_device(s.cuda(), plan)
    assert rep.auc == auc and torch.equal(per_t2, per_t_dev) and np.array_equal(gt, plan.gt)


def test_two_routes_from_window_scores_are_bitwise_equal():
    s, plan, rep, *_ = _end_to_end()
    rep2, _, _ = E.score_report_device(s.cuda(), plan)
    assert rep2.auc == rep.auc and list(rep2.lines()) == list(rep.lines())
    np.testing.assert_array_equal(rep2.clip_auc, rep.clip_auc)
    np.testing.assert_array_equal(rep2.frame_scores, rep.frame_scores)


def test_lit_encoder_with_the_key(monkeypatch):
    from coskad_amd.lit import LitEncoder
    (s, trans, meta, frames, gts), kw = _mixed_case()
    lit = LitEncoder(_args(pad_size=kw["pad_size"]))
    lit.gts, lit.hr_masks = gts, kw["hr_masks"]
    auc = lit._score_windows(s.cuda(), trans, meta, frames)
    assert not hasattr(lit, "last_report") and "validation_clip_auc_mean" not in lit.logged
    lit.args.eval_report = True
    calls = []
    real = E.score_report
    monkeypatch.setattr(E, "score_report", lambda *a, **k: (calls.append("host"), real(*a, **k))[1])
    assert lit._score_windows(s.cuda(), trans, meta, frames) == auc and calls == []          # the device route, the same AUC
    rep = lit.last_report
    assert rep.auc == auc == lit.logged["validation_auc"] and rep.clip_auc.shape == (2, len(gts))
    assert lit.logged["validation_clip_auc_mean"] == np.nanmean(rep.clip_auc_mean_t)
    np.testing.assert_array_equal(rep.clip_auc, _end_to_end()[2].clip_auc)
    lit.args.device_scoring = False                            # the host route builds the host report
    auc_host = lit._score_windows(s.cuda(), trans, meta, frames)
    assert calls == ["host"] and lit.last_report is not rep
    np.testing.assert_allclose(lit.last_report.clip_auc, rep.clip_auc, rtol=1e-10, atol=0)
    np.testing.assert_allclose(auc_host, auc, rtol=1e-10)


def test_eval_cli_prints_the_report(tmp_path):
    from argparse import Namespace

    from coskad_amd.lit import LitEncoder, Trainer, save_checkpoint
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), load_ckpt="init.ckpt", create_experiment_dir=False)
    assert "eval_report" not in cfg
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(0)
    lit = LitEncoder(args).cuda()
    ckdir = os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"])
    os.makedirs(ckdir)
    save_checkpoint(lit, os.path.join(ckdir, "init.ckpt"))      # an untrained model: the test is about the log, not the score
    path = str(tmp_path / "eval.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    # the value the evaluation prints today: the same checkpoint scored in-process, without the key
    test, gts = make_dataset(n_scenes=2, n_clips=3, n_persons=3, clip_len=200, num_transform=args.dataset_num_transform, anomaly=True,
                             seed=args.seed + 1, T=args.dataset_seg_len)
    lit.gts = gts
    auc_plain = lit.validation_epoch_end(Trainer().predict(lit, lambda: batches(test, args.dataset_batch_size)))
    assert not hasattr(lit, "last_report")
    r = subprocess.run([sys.executable, "eval_COSKAD.py", "--config", path, "--report", "--report-dir", str(tmp_path / "rep")], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    final = re.findall(r"^final AUC score: (\S+)$", r.stdout, flags=re.M)
    assert final == [str(float(auc_plain))]                    # the line and its value are unchanged
    lines = r.stdout.splitlines()
    nt = cfg["dataset_num_transform"]
    clip_lines = [l for l in lines if re.match(r"^transf: \d+/%d, clip: \(\d+, \d+\),\d+/6, score: \S+ average_score: \S+$" % nt, l)]
    assert len(clip_lines) == nt * 6 and not any(l.startswith("{") for l in lines)
    assert [l for l in lines if l.startswith("Test set score for transformation")] == [f"Test set score for transformation {t + 1}"
                                                                                        for t in range(nt)]
    assert len([l for l in lines if l.startswith("auc = ")]) == nt and lines[-1].startswith("final AUC score: ")
    rep = json.load(open(tmp_path / "rep" / "report.json"))
    assert str(rep["auc"]) == final[0] and len(rep["clip_keys"]) == 6
    assert np.load(tmp_path / "rep" / "1_1.npy").shape == (200,)
