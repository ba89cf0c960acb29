"""The evaluation report on the host (eval_utils.score_report / roc_crossing_thresholds: the reference's loops, eval_COSKAD.py:222-242,
utils/eval_utils.py:216-230) against direct scikit-learn calls, the C ABI of csrc/score_report.hip without a GPU, and the `eval_report`
key's default: absent means that no report function runs."""
import ctypes
import json
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score, roc_curve

from coskad_amd import _lib
from coskad_amd.utils import eval_utils as E
from coskad_amd.utils import score_plan as SP
from coskad_amd.utils.synthetic import make_dataset

CLIP_NAMES = "ABCDEFGH"
CLIP_LENGTHS = (1, 2, 37, 256, 257, 1000, 9000, 0)
UNDEFINED = {"A", "C", "H"}


def crafted_report_case(nt=3, seed=0):
    """-> (per_t [nt, F], gt [F], segments [8, 2], clip keys): eight clips in one vector, every length at or just beyond an edge.
    A one frame; B a positive and a negative of equal score; C 37 negatives; D 256 mixed labels, one score; E 257 scores rounded to one
    decimal; F 1 000 continuous; G 9 000 with ties (35 tiles of 256 and a part); H empty, as a human-related mask can leave a clip."""
    rng = np.random.default_rng(seed)
    ends = np.cumsum(CLIP_LENGTHS)
    seg = np.stack([ends - CLIP_LENGTHS, ends], 1)
    F = int(ends[-1])
    gt = np.zeros(F, dtype=np.int64)
    per_t = np.zeros((nt, F))
    sl = {n: slice(*seg[i]) for i, n in enumerate(CLIP_NAMES)}
    gt[sl["A"]] = 1
    gt[sl["B"]] = [1, 0]
    gt[sl["D"]] = rng.integers(0, 2, 256); gt[sl["D"]][:2] = [0, 1]
    gt[sl["E"]] = rng.integers(0, 2, 257); gt[sl["E"]][:2] = [0, 1]
    gt[sl["F"]] = rng.random(1000) < 0.3
    gt[sl["G"]] = rng.random(9000) < 0.1
    for t in range(nt):
        per_t[t, sl["A"]] = rng.random()
        per_t[t, sl["B"]] = rng.random()
        per_t[t, sl["C"]] = rng.random(37)
        per_t[t, sl["D"]] = rng.random()
        per_t[t, sl["E"]] = np.round(rng.random(257), 1)
        per_t[t, sl["F"]] = rng.random(1000) + 0.2 * gt[sl["F"]]
        per_t[t, sl["G"]] = np.round(rng.random(9000) + 0.3 * gt[sl["G"]], 2)
    return per_t, gt, seg, [(1, i + 1) for i in range(8)]


def sklearn_clip_auc(y, s):
    """roc_auc_score of a clip, NaN where scikit-learn has no answer: it raises there (before 1.6) or warns and returns NaN"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return float(roc_auc_score(y, s)) if len(y) else float("nan")
    except ValueError:
        return float("nan")


def check_crafted_fixture(per_t, gt, seg):
    """the properties the fixture is built for, by scikit-learn alone"""
    for t in range(per_t.shape[0]):
        aucs = {n: sklearn_clip_auc(gt[a:b], per_t[t, a:b]) for n, (a, b) in zip(CLIP_NAMES, seg.tolist())}
        assert {n for n, v in aucs.items() if np.isnan(v)} == UNDEFINED, aucs
        assert aucs["B"] == 0.5 and aucs["D"] == 0.5
        a, b = seg[4]
        e, ye = per_t[t, a:b], gt[a:b]
        assert len(set(e[ye == 1]) & set(e[ye == 0])) >= 5           # E: ties across the labels
        a, b = seg[6]
        assert b - a > 8192 and len(np.unique(per_t[t, a:b])) < 200   # G: longer than 64 KB of doubles, heavy ties
    assert [b - a for a, b in seg.tolist()] == list(CLIP_LENGTHS)


def find_threshold_rows(seed=0, F=48):
    """-> (rows [3, F], gt [F]) found by a seeded search with scikit-learn: row 0 separates the classes perfectly with the positives
    at one score, so its first point is already the corner (0, 1) and the first threshold is inf; row 1 has a point exactly on tpr = 1 - fpr (two finite thresholds); row 2 is a case where drop_intermediate
    changes the thresholds."""
    rng = np.random.default_rng(seed)
    gt = np.zeros(F, dtype=np.int64)
    gt[rng.permutation(F)[:F // 2]] = 1
    perfect = np.where(gt == 1, 0.9, rng.random(F) * 0.4)

    def crossing(s, drop):
        fpr, tpr, tr = roc_curve(gt, s, drop_intermediate=drop)
        return tr[np.argwhere(np.diff(np.sign(tpr - (1 - fpr)))).flatten()]
    two = dropped = None
    for _ in range(2000):
        s = np.round(rng.random(F) + 0.3 * gt, 1 if two is None else 2)
        if two is None and len(crossing(s, True)) == 2 and np.isfinite(crossing(s, True)).all():
            two = s
        elif two is not None and dropped is None and not np.array_equal(crossing(s, True), crossing(s, False)):
            dropped = s
        if two is not None and dropped is not None:
            break
    assert two is not None and dropped is not None
    assert crossing(perfect, True).tolist() == [np.inf, 0.9]
    return np.stack([perfect, two, dropped], 0), gt


def test_crafted_fixture_has_its_properties():
    per_t, gt, seg, _ = crafted_report_case()
    check_crafted_fixture(per_t, gt, seg)
    rows, y = find_threshold_rows()
    assert rows.shape == (3, 48) and 0 < y.sum() < 48


def test_score_report_matches_sklearn_on_the_crafted_fixture():
    per_t, gt, seg, keys = crafted_report_case()
    rep = E.score_report(per_t, gt, seg, keys)
    nt = per_t.shape[0]
    pds = np.mean(per_t, 0)
    assert rep.auc == roc_auc_score(gt, pds) and isinstance(rep.auc, float)
    assert rep.clip_keys == keys and rep.clip_auc.shape == (nt, 8) and rep.n_pos.dtype == np.int64
    for t in range(nt):
        assert rep.auc_t[t] == roc_auc_score(gt, per_t[t])
        want = np.array([sklearn_clip_auc(gt[a:b], per_t[t, a:b]) for a, b in seg.tolist()])
        np.testing.assert_array_equal(rep.clip_auc[t], want)
        assert {CLIP_NAMES[i] for i in np.nonzero(np.isnan(rep.clip_auc[t]))[0]} == UNDEFINED
        np.testing.assert_array_equal(rep.clip_auc_mean_t[t], np.nanmean(want))
        fpr, tpr, tr = roc_curve(gt, per_t[t])
        np.testing.assert_array_equal(rep.thresholds_t[t], tr[np.argwhere(np.diff(np.sign(tpr - (1 - fpr)))).flatten()])
        assert 1 <= len(rep.thresholds_t[t]) <= 2
    np.testing.assert_array_equal(rep.clip_auc_final, [sklearn_clip_auc(gt[a:b], pds[a:b]) for a, b in seg.tolist()])
    np.testing.assert_array_equal(rep.n_pos, [int(gt[a:b].sum()) for a, b in seg.tolist()])
    np.testing.assert_array_equal(rep.n_pos + rep.n_neg, CLIP_LENGTHS)
    # a dict of rows, as score_dataset returns them, is the same report
    rep2 = E.score_report({t: per_t[t] for t in range(nt)}, gt, seg, keys)
    np.testing.assert_array_equal(rep2.clip_auc, rep.clip_auc)
    assert rep2.auc == rep.auc


def test_roc_crossing_thresholds_edge_rows():
    rows, gt = find_threshold_rows()
    thr = [E.roc_crossing_thresholds(gt, r) for r in rows]
    assert thr[0].tolist() == [np.inf, 0.9] and len(thr[1]) == 2 and np.isfinite(thr[1]).all()
    fpr, tpr, tr = roc_curve(gt, rows[2], drop_intermediate=False)
    assert not np.array_equal(thr[2], tr[np.argwhere(np.diff(np.sign(tpr - (1 - fpr)))).flatten()])
    np.testing.assert_array_equal(E.roc_crossing_thresholds([0, 1], [0.1, 0.9]), [np.inf, 0.9])
    for r, t in zip(rows, thr):
        assert np.isin(t[np.isfinite(t)], r).all()                   # each value bit-equal to a score
    assert E.roc_crossing_thresholds([1, 1, 1], [0.1, 0.2, 0.3]).shape == (0,)


def test_all_clips_undefined_gives_nan_mean():
    rep = E.score_report(np.array([[0.1, 0.2, 0.3, 0.4]]), [0, 0, 1, 1], [[0, 2], [2, 4]], [(1, 1), (1, 2)])
    assert np.isnan(rep.clip_auc).all() and np.isnan(rep.clip_auc_mean_t[0]) and rep.auc == 1.0


def test_segments_are_checked():
    for bad in ([[0, 5]], [[-1, 2]], [[2, 1]], [[0, 3], [2, 4]]):
        with pytest.raises(ValueError, match="segments"):
            E.score_report(np.zeros((1, 4)), [0, 1, 0, 1], bad, [(1, 1)] * len(bad))


def test_lines_and_save(tmp_path):
    per_t, gt, seg, keys = crafted_report_case()
    rep = E.score_report(per_t, gt, seg, keys)
    lines = list(rep.lines())
    assert not any(l.startswith("{") for l in lines) and all("\n" not in l for l in lines)
    assert lines[-1] == "final AUC score: {}".format(rep.auc)
    assert len(lines) == 3 * (8 + 3) + 1
    assert lines[0].startswith("transf: 1/3, clip: (1, 1),1/8, score: nan average_score: nan")
    assert lines[1] == "transf: 1/3, clip: (1, 2),2/8, score: 0.5 average_score: 0.5"
    assert lines[2] == "transf: 1/3, clip: (1, 3),3/8, score: nan average_score: 0.5"         # undefined: nan, not a stale value
    assert lines[7].endswith("average_score: {}".format(rep.clip_auc_mean_t[0]))
    assert lines[8] == "Test set score for transformation 1" and lines[10] == "auc = {}".format(rep.auc_t[0])
    assert lines[9] == str(rep.thresholds_t[0])
    rep.save(str(tmp_path / "r"))
    d = json.load(open(tmp_path / "r" / "report.json"))
    assert d["auc"] == rep.auc and d["clip_auc"][0][0] is None and d["clip_auc"][1][4] == rep.clip_auc[1, 4]
    assert d["clip_keys"][6] == [1, 7] and d["n_pos"] == rep.n_pos.tolist()
    np.testing.assert_array_equal(np.load(tmp_path / "r" / "1_7.npy"), np.mean(per_t, 0)[seg[6, 0]:seg[6, 1]])
    assert np.load(tmp_path / "r" / "1_8.npy").shape == (0,)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------

REPORT_SYMBOLS = ("coskad_score_report_tile", "coskad_score_report_auc_ws", "coskad_score_report_thr_ws", "coskad_score_report_auc_f64",
                  "coskad_score_report_thresholds_f64")


def test_report_symbols_are_declared_and_exported():
    protos = _lib.prototypes()
    lib = _lib.lib()
    for name in REPORT_SYMBOLS:
        assert name in protos and getattr(lib, name).argtypes == protos[name][1], name
    assert lib.coskad_score_report_tile() == SP.REPORT_TILE == 256
    assert lib.coskad_score_report_auc_ws(4, 10) == 40 and lib.coskad_score_report_auc_ws(0, 10) == 0
    assert lib.coskad_score_report_thr_ws(3, 257) == 12 and lib.coskad_score_report_thr_ws(3, 0) == 0
    assert protos["coskad_score_report_auc_ws"][0] is ctypes.c_longlong


def test_report_argument_errors_are_reported_without_a_gpu():
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def auc(*ptrs, ws=64, n_tiles=3, n_rows=2, n_seg=2, F=300):
        _lib.call("coskad_score_report_auc_f64", *ptrs, ws, n_tiles, n_rows, n_seg, F, null)

    def thr(*ptrs, ws=64, n_rows=2, F=300):
        _lib.call("coskad_score_report_thresholds_f64", *ptrs, ws, n_rows, F, null)
    for i in range(7):
        with pytest.raises(_lib.CoskadHipError, match="null pointer"):
            auc(*[null if j == i else p for j in range(7)])
    for i in range(4):
        with pytest.raises(_lib.CoskadHipError, match="null pointer"):
            thr(*[null if j == i else p for j in range(4)])
    for kw in (dict(n_rows=0), dict(n_seg=0), dict(F=0), dict(n_tiles=0), dict(F=-5), dict(n_seg=-1)):
        with pytest.raises(_lib.CoskadHipError, match=r"n_rows=.* n_seg=.* F="):
            auc(*[p] * 7, **kw)
    with pytest.raises(_lib.CoskadHipError, match="tiles for 2 segments"):
        auc(*[p] * 7, n_tiles=4)                                     # 300 frames in 2 segments: 3 tiles at the most
    with pytest.raises(_lib.CoskadHipError, match=r"\(-4\).*workspace of 5 elements, 6 needed"):
        auc(*[p] * 7, ws=5)
    for kw in (dict(n_rows=0), dict(F=0), dict(n_rows=-1)):
        with pytest.raises(_lib.CoskadHipError, match=r"n_rows=.* F="):
            thr(*[p] * 4, **kw)
    with pytest.raises(_lib.CoskadHipError, match=r"\(-4\).*workspace of 7 elements, 8 needed"):
        thr(*[p] * 4, ws=7)


def test_device_report_refuses_host_tensors_and_bad_segments():
    per_t, gt, seg, keys = crafted_report_case(nt=1)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        SP.report_from_frame_scores(torch.from_numpy(per_t), torch.from_numpy(per_t[0]), torch.from_numpy(gt).int(),
                                    torch.from_numpy(seg).int(), keys)
    with pytest.raises(ValueError, match="segments"):
        SP.check_segments([[0, 4], [3, 6]], 6)
    key, tile_ptr, whole, whole_ptr = SP.report_tables(seg, int(seg[-1, 1]))
    assert tile_ptr.tolist() == [0, 1, 2, 3, 4, 6, 10, 46, 46] and whole.tolist() == [[0, 10553]] and whole_ptr.tolist() == [0, 42]
    assert tile_ptr[-1] <= 10553 // 256 + 8 and key.dtype == torch.int32
    np.testing.assert_array_equal(key.numpy()[[0, 1, 2, 3, 39, 40, 10552]], [1, 3, 3, 5, 5, 7, 13])


# ---- the key's default ------------------------------------------------------------------------------------------------------------

def _args(**kw):
    a = dict(num_coords=2, h_dim=16, latent_dim=8, dataset_seg_len=12, dropout=0, channels=[16, 8, 16], projector="linear",
             encoder_type="STS_GCN", hyperbolic=False, static_center=False, center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6,
             dataset_batch_size=256, dataset_num_transform=2, dataset_headless=False, dataset_kp18_format=False, smoothing=50,
             dataset_choice="UBnormal", validation=True)
    a.update(kw)
    return Namespace(**a)


def test_without_the_key_no_report_function_runs(monkeypatch):
    from coskad_amd.lit import LitEncoder
    (x, trans, meta, frames), gts = make_dataset(n_scenes=1, n_clips=3, n_persons=2, clip_len=80, num_transform=2, seed=4)
    s = torch.rand(x.shape[0], generator=torch.Generator().manual_seed(0), dtype=torch.float64) + 0.05
    calls = []
    for mod in (E, SP):
        for name in ("score_report", "score_report_device", "report_from_frame_scores", "roc_crossing_thresholds", "clip_segments",
                     "ScoreReport"):
            if hasattr(mod, name):
                real = getattr(mod, name)
                monkeypatch.setattr(mod, name, lambda *a, _real=real, _n=name, **k: (calls.append(_n), _real(*a, **k))[1])
    args = _args()
    assert not hasattr(args, "eval_report")
    lit = LitEncoder(args)
    lit.gts = gts
    auc = lit._score_windows(s, trans, meta, frames)                 # scores on the host: the host route
    assert calls == [] and not hasattr(lit, "last_report") and "validation_clip_auc_mean" not in lit.logged
    args.eval_report = False
    assert lit._score_windows(s, trans, meta, frames) == auc and calls == [] and not hasattr(lit, "last_report")
    args.eval_report = True
    assert lit._score_windows(s, trans, meta, frames) == auc         # the same validation_auc with the key
    assert "score_report" in calls and "score_report_device" not in calls
    rep = lit.last_report
    assert rep.auc == auc == lit.logged["validation_auc"] and rep.clip_keys == sorted(gts)
    assert lit.logged["validation_clip_auc_mean"] == np.nanmean(rep.clip_auc_mean_t)
    keys, seg = E.clip_segments(gts)
    for t in range(2):
        np.testing.assert_array_equal(rep.clip_auc[t], [sklearn_clip_auc(lit_gt, lit.last_scores[t][a:b])
                                                        for (a, b), lit_gt in zip(seg.tolist(), (gts[k] for k in keys))])
