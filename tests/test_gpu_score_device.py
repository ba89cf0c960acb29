"""Frame-level scoring on the device (csrc/score_frames.hip through coskad_amd.ops and eval_utils.score_dataset_device) against the
loop-for-loop oracle of the reference's scoring (oracle/ref_scoring.py), scipy and sklearn: each stage kernel alone, the whole route on
the cases of tests/test_scoring.py, and the route LitEncoder takes."""
from argparse import Namespace

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score

from coskad_amd import ops
from coskad_amd.utils import eval_utils as E
from coskad_amd.utils import score_plan as SP
from coskad_amd.utils.synthetic import batches, make_dataset
from oracle import ref_scoring as RS

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-12)          # tests/test_scoring.py's own


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda()


# ---- stage kernels alone ------------------------------------------------------------------------------------------------------

def test_padding_matches_reference_branches():
    rng = np.random.default_rng(0)
    rows, pads = [], []
    for trial in range(200):                                   # the rows of test_pad_scores_matches_reference_branches
        n = int(rng.integers(5, 60))
        v = rng.random(n)
        for _ in range(int(rng.integers(0, 4))):               # random absence intervals, incl. at both ends
            a = int(rng.integers(0, n)); b = int(rng.integers(a, min(n, a + 15)))
            v[a:b + 1] = 0
        rows.append(v); pads.append(int(rng.integers(0, 8)))
    big = rng.random(40)
    big[[0, 1, 17, 18, 19, 38]] = 0
    rows += [big, big.copy(), np.zeros(12), np.zeros(2), rng.random(1)]
    pads += [41, 25, 3, 3, 3]                                  # pad larger than the row; frame n-1 zeroed by a run that is not its nearest
    row_ptr = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])])
    n_max = max(r.shape[0] for r in rows)
    pads = np.array(pads)
    for pad in sorted(set(pads.tolist())):                     # one pad size per launch: the rows of that size
        sel = np.nonzero(pads == pad)[0]
        ptr = np.concatenate([[0], np.cumsum([rows[i].shape[0] for i in sel])])
        pf = torch.from_numpy(np.concatenate([rows[i] for i in sel])).cuda()
        got = ops.score_pad_(pf, _i32(ptr), pad, n_max).cpu().numpy()
        for j, i in enumerate(sel):
            want = RS.pad_scores(rows[i].copy(), np.zeros(rows[i].shape[0]), pad)
            np.testing.assert_array_equal(got[ptr[j]:ptr[j + 1]], want, err_msg=str((i, rows[i], pad)))
    assert row_ptr[-1] > 0


SEG_LENGTHS = (0, 1, 5, 11, 12, 60, 121, 241, 300, 1000)


def test_smoothing_matches_score_process_per_segment():
    rng = np.random.default_rng(1)
    bounds = np.cumsum((0,) + SEG_LENGTHS)
    segs = np.stack([bounds[:-1], bounds[1:]], 1)
    raw = rng.random((3, int(bounds[-1])))
    raw[:, rng.integers(0, raw.shape[1], 200)] = 0.0
    tiles = SP.segment_tiles(segs)
    assert tiles.shape[0] == sum(-(-m // SP.TILE) for m in SEG_LENGTHS)
    per_t, mean = ops.score_smooth(torch.from_numpy(raw).cuda(), _i32(tiles), torch.from_numpy(E.gaussian_taps()).cuda())
    per_t, mean = per_t.cpu().numpy(), mean.cpu().numpy()
    for t in range(3):
        want = np.concatenate([RS.score_process(raw[t, a:b]) for a, b in segs])
        np.testing.assert_allclose(per_t[t], want, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(mean, np.mean(per_t, 0))


def _auc_case(kind, F=5000):
    rng = np.random.default_rng(2)
    gt = (rng.random(F) < 0.3).astype(np.int64)
    s = rng.random(F) + 0.3 * gt
    if kind == "quantised":
        s = np.floor(s * 8 / 1.3) / 8                          # 8 levels: heavy ties
    elif kind == "equal":
        s = np.full(F, 0.25)
    return s, gt


@pytest.mark.parametrize("kind", ["continuous", "quantised", "equal"])
def test_auc_matches_sklearn(kind):
    s, gt = _auc_case(kind)
    got = E.auc_device(torch.from_numpy(s).cuda(), _i32(gt))
    np.testing.assert_allclose(got, roc_auc_score(gt, s), rtol=1e-12)
    if kind == "equal":
        assert got == 0.5
    if kind == "quantised":
        assert np.unique(s).shape[0] <= 9


def test_auc_of_a_single_class_raises():
    s = torch.rand(300, dtype=torch.float64).cuda()
    for gt in (np.zeros(300), np.ones(300)):
        with pytest.raises(ValueError, match="Only one class"):
            E.auc_device(s, _i32(gt))


def test_person_frames_skip_exact_zeros_in_both_precisions():
    (x, trans, meta, frames), gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, seed=4)
    plan = E.ScorePlan(trans, meta, frames, gts, 1, device="cuda")
    s = torch.rand(x.shape[0], dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    s[::5] = 0.0
    for dtype in (torch.float64, torch.float32):
        sc = s.to(dtype)
        pf = ops.score_person_frames(sc.cuda(), plan.win_ptr, plan.win_idx).cpu().numpy()
        for p, (t, scene, clip, person) in enumerate(plan.person_keys.tolist()):
            sel = ((meta[:, 0] == scene) & (meta[:, 1] == clip) & (meta[:, 2] == person)).numpy()
            mat = RS.windows_to_frames(sc.double().numpy()[sel], frames.numpy()[sel], 80)
            cnt = (mat != 0).sum(0)
            want = np.where(cnt > 0, mat.sum(0) / np.maximum(cnt, 1), 0.0)
            np.testing.assert_allclose(pf[plan.row_ptr[p]:plan.row_ptr[p + 1]], want, rtol=1e-14, atol=0)


# ---- the whole route ---------------------------------------------------------------------------------------------------------

def _base_case():
    (x, trans, meta, frames), gts = make_dataset(n_scenes=2, n_clips=2, n_persons=3, clip_len=90, num_transform=2, seed=3)
    s = torch.rand(x.shape[0], generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    s[::37] = 0.0                                              # exact zeros count as 'missing' in the reference
    return (s, trans, meta, frames, gts), dict(num_transform=2)


def _missing_clip_case():
    (x, trans, meta, frames), gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, seed=5)
    keep = ~((meta[:, 1] == 2) & (meta[:, 2] == 1))            # clip 2 keeps a single person
    keep &= ~((meta[:, 1] == 1) & (meta[:, 3] > 30))           # clip 1: no window covers the late frames
    x, trans, meta, frames = x[keep], trans[keep], meta[keep], frames[keep]
    s = torch.rand(x.shape[0], dtype=torch.float64, generator=torch.Generator().manual_seed(1)) + 0.1
    return (s, trans, meta, frames, gts), dict(num_transform=1)


def _ragged_case(seed=7):
    (x, trans, meta, frames), gts = make_dataset(n_scenes=2, n_clips=2, n_persons=3, clip_len=100, num_transform=2, seed=seed)
    keep = ~((meta[:, 0] == 1) & (meta[:, 1] == 1) & (meta[:, 2] == 1) & (meta[:, 3] > 25) & (meta[:, 3] < 60))
    keep &= ~((meta[:, 0] == 2) & (meta[:, 1] == 2) & (meta[:, 2] == 2) & (meta[:, 3] < 40))
    keep &= ~((meta[:, 0] == 1) & (meta[:, 1] == 2) & (meta[:, 2] == 0))
    x, trans, meta, frames = x[keep], trans[keep], meta[keep], frames[keep]
    s = torch.rand(x.shape[0], dtype=torch.float64, generator=torch.Generator().manual_seed(seed)) + 0.05
    return s, trans, meta, frames, gts


def _hr():
    rng = np.random.default_rng(1)
    return {(1, 1): rng.random(100) > 0.3, (2, 2): rng.random(100) > 0.5}


def _mixed_case():
    (xa, ta, ma, fa), ga = make_dataset(2, 2, 2, clip_len=72, T=8, num_transform=2, seed=11)
    (xb, tb, mb, fb), gb = make_dataset(1, 2, 3, clip_len=300, T=8, num_transform=2, seed=12)
    mb = mb.clone()
    mb[:, 0] += 2
    gts = dict(ga)
    gts.update({(k[0] + 2, k[1]): v for k, v in gb.items()})
    trans, meta, frames = torch.cat([ta, tb]), torch.cat([ma, mb]), torch.cat([fa, fb])
    s = torch.rand(trans.shape[0], generator=torch.Generator().manual_seed(3), dtype=torch.float64) + 0.05
    s[::53] = 0.0
    few = np.zeros(72, dtype=bool)
    few[[3, 10, 20, 21, 40, 60, 71]] = True                    # 7 frames: shorter than the 11-frame shift
    hr = {(1, 1): few, (3, 2): np.random.default_rng(5).random(300) > 0.4}
    return (s, trans, meta, frames, gts), dict(num_transform=2, pad_size=6, hr_masks=hr)


CASES = {
    "base": _base_case,
    "missing_clip": _missing_clip_case,
    "pad10": lambda: (_ragged_case(), dict(num_transform=2, pad_size=10)),
    "hr": lambda: (_ragged_case(), dict(num_transform=2, pad_size=-1, hr_masks=_hr())),
    "hr_pad4": lambda: (_ragged_case(), dict(num_transform=2, pad_size=4, hr_masks=_hr())),
    "mixed": _mixed_case,
}
_memo = {}


def _case(name):
    """(inputs, settings, the oracle's result, the device route's result): computed once, shared, left unchanged"""
    if name not in _memo:
        (s, trans, meta, frames, gts), kw = CASES[name]()
        ref = RS.score_dataset(s.numpy(), trans.numpy(), meta.numpy(), frames.numpy(), gts, kw["num_transform"],
                               pad_size=kw.get("pad_size", -1), hr_masks=kw.get("hr_masks"))
        plan = E.ScorePlan(trans, meta, frames, gts, device="cuda", **kw)
        auc, per_t, gt = E.score_dataset_device(s.cuda(), plan)
        assert per_t.is_cuda and per_t.dtype == torch.float64 and per_t.shape == (kw["num_transform"], plan.F)
        _memo[name] = ((s, trans, meta, frames, gts), kw, ref, (auc, per_t.cpu().numpy(), gt), plan)
    return _memo[name]


def _class_gap(pds, gt):
    """smallest |positive score - negative score| relative to the largest score"""
    pos, neg = np.sort(pds[gt != 0]), np.sort(pds[gt == 0])
    i = np.searchsorted(neg, pos)
    below, above = neg[np.maximum(i - 1, 0)], neg[np.minimum(i, neg.shape[0] - 1)]
    return float(np.minimum(np.abs(pos - below), np.abs(pos - above)).min() / np.abs(pds).max())


@pytest.mark.parametrize("name", ["base", "missing_clip", "pad10", "hr", "hr_pad4"])
def test_route_matches_reference_loops(name):
    _, kw, (auc_r, per_t_r, gt_r), (auc, per_t, gt), _ = _case(name)
    assert np.array_equal(gt, gt_r) and gt.dtype == gt_r.dtype
    for t in range(kw["num_transform"]):
        np.testing.assert_allclose(per_t[t], per_t_r[t], **TOL)
    # no positive / negative pair of the oracle's averaged score is close enough for a rank to flip at the tolerance above
    gap = _class_gap(np.mean(np.stack([per_t_r[t] for t in range(kw["num_transform"])], 0), 0), gt_r)
    assert gap >= 1e-9, gap
    np.testing.assert_allclose(auc, auc_r, rtol=1e-12)


def test_mixed_clip_lengths_with_padding_and_masks():
    """clips of 72 and 300 frames in one table (two tiles per long clip, segments shorter than the filter's halo and than the shift),
    pad 6, a 7-frame and a random human-related mask.  The oracle's averaged score has exact positive / negative ties here, so the
    AUC is compared with sklearn's on the device route's own averaged vector."""
    _, kw, (auc_r, per_t_r, gt_r), (auc, per_t, gt), plan = _case("mixed")
    assert plan.segments[0].tolist() == [0, 7] and plan.n_tiles == 1 + 3 + 2 + 1 and int(plan.person_n.max()) == 300
    assert np.array_equal(gt, gt_r)
    for t in range(2):
        np.testing.assert_allclose(per_t[t], per_t_r[t], **TOL)
    np.testing.assert_allclose(auc, roc_auc_score(gt, np.mean(per_t, 0)), rtol=1e-12)


def test_float32_scores_are_widened_on_load():
    (s, trans, meta, frames, gts), kw, _, _, plan = _case("hr_pad4")
    s32 = s.float()
    auc, per_t, _ = E.score_dataset_device(s32.cuda(), plan)
    _, per_t_r, _ = RS.score_dataset(s32.double().numpy(), trans.numpy(), meta.numpy(), frames.numpy(), gts, 2, pad_size=4,
                                     hr_masks=kw["hr_masks"])
    for t in range(2):
        np.testing.assert_allclose(per_t[t].cpu().numpy(), per_t_r[t], **TOL)


def test_two_runs_are_bitwise_equal():
    (s, *_), _, _, (auc, per_t, _), plan = _case("mixed")
    auc2, per_t2, _ = E.score_dataset_device(s.cuda(), plan)
    assert auc2 == auc and np.array_equal(per_t2.cpu().numpy(), per_t)


def test_route_refuses_scores_of_another_table():
    (s, *_), _, _, _, plan = _case("base")
    with pytest.raises(ValueError, match="window scores for a plan"):
        E.score_dataset_device(s[:-1].cuda(), plan)


# ---- through LitEncoder ------------------------------------------------------------------------------------------------------

def _args(**kw):
    a = dict(num_coords=2, h_dim=16, latent_dim=8, dataset_seg_len=12, dropout=0, channels=[16, 8, 16], projector="linear",
             encoder_type="STS_GCN", hyperbolic=False, static_center=False, center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6,
             dataset_batch_size=256, dataset_num_transform=2, dataset_headless=False, dataset_kp18_format=False, smoothing=50,
             dataset_choice="UBnormal", validation=True)
    a.update(kw)
    return Namespace(**a)


def test_plan_is_reused_for_the_same_table_and_rebuilt_for_a_permuted_one():
    from coskad_amd.lit import LitEncoder
    (s, trans, meta, frames, gts), _, (auc_r, per_t_r, _), _, _ = _case("base")
    lit = LitEncoder(_args())
    lit.gts = gts
    auc = lit._score_windows(s.cuda(), trans, meta, frames)
    plan = lit._score_plan
    assert lit._score_windows(s.cuda(), trans.clone(), meta.clone(), frames.clone()) == auc and lit._score_plan is plan
    np.testing.assert_allclose(auc, auc_r, rtol=1e-12)
    perm = torch.randperm(s.shape[0], generator=torch.Generator().manual_seed(0))
    auc_p = lit._score_windows(s[perm].cuda(), trans[perm], meta[perm], frames[perm])
    assert lit._score_plan is not plan and lit._score_plan.matches(trans[perm], meta[perm], frames[perm])
    np.testing.assert_allclose(auc_p, auc_r, rtol=1e-12)       # the same windows in another order: the same frames
    assert isinstance(lit.last_scores, dict) and sorted(lit.last_scores) == [0, 1]
    for t in range(2):
        assert isinstance(lit.last_scores[t], np.ndarray)
        np.testing.assert_allclose(lit.last_scores[t], per_t_r[t], **TOL)
    lit.args.pad_size = 10                                     # another setting on the same table: a new plan as well
    plan = lit._score_plan
    lit._score_windows(s[perm].cuda(), trans[perm], meta[perm], frames[perm])
    assert lit._score_plan is not plan and lit._score_plan.pad_size == 10


def test_validation_with_and_without_device_scoring(tmp_path):
    from coskad_amd.lit import LitEncoder, Trainer
    torch.manual_seed(0)
    train, _ = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=False, seed=1)
    test, gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=True, seed=2)
    args = _args()
    assert not hasattr(args, "device_scoring")                 # an optional key: on unless the yaml says false
    lit = LitEncoder(args).cuda()
    lit.gts = gts
    tr = Trainer(max_epochs=1, ckpt_dir=None)
    tr.fit(lit, lambda: batches(train, 256, shuffle=True, seed=0), lambda: batches(test, 512))
    auc_dev, scores_dev = tr.history[-1]["validation_auc"], lit.last_scores
    assert getattr(lit, "_score_plan", None) is not None and lit._score_plan.N == test[0].shape[0]
    args.device_scoring = False
    plan = lit._score_plan
    auc_host = tr.validate(lit, lambda: batches(test, 512))
    scores_host = lit.last_scores
    assert lit._score_plan is plan and scores_host is not scores_dev
    assert sorted(scores_dev) == sorted(scores_host) == [0, 1]
    for t in range(2):
        np.testing.assert_allclose(scores_dev[t], scores_host[t], rtol=1e-10, atol=0)
    gap = _class_gap(np.mean(np.stack([scores_host[0], scores_host[1]], 0), 0), plan.gt)
    assert gap >= 1e-9, gap
    np.testing.assert_allclose(auc_dev, auc_host, rtol=1e-12)
