"""ScorePlan (coskad_amd/utils/score_plan.py): the index tables the scoring kernels read, derived once from a window table -- against
the window table itself and the loop-for-loop oracle (oracle/ref_scoring.py).  Also what the scoring entry points of the C ABI say
before they touch a device.  No kernel runs."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter1d

from coskad_amd import _lib
from coskad_amd.utils import eval_utils as E
from coskad_amd.utils import score_plan as SP
from coskad_amd.utils.synthetic import make_dataset
from oracle import ref_scoring as RS


def _base_case():
    (x, trans, meta, frames), gts = make_dataset(n_scenes=2, n_clips=2, n_persons=3, clip_len=90, num_transform=2, seed=3)
    return trans, meta, frames, gts


def _missing_clip_case():
    (x, trans, meta, frames), gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, seed=5)
    keep = ~((meta[:, 1] == 2) & (meta[:, 2] == 1))
    keep &= ~((meta[:, 1] == 1) & (meta[:, 3] > 30))
    return trans[keep], meta[keep], frames[keep], gts


def _ragged_case(seed=7):
    (x, trans, meta, frames), gts = make_dataset(n_scenes=2, n_clips=2, n_persons=3, clip_len=100, num_transform=2, seed=seed)
    keep = ~((meta[:, 0] == 1) & (meta[:, 1] == 1) & (meta[:, 2] == 1) & (meta[:, 3] > 25) & (meta[:, 3] < 60))
    keep &= ~((meta[:, 0] == 2) & (meta[:, 1] == 2) & (meta[:, 2] == 2) & (meta[:, 3] < 40))
    keep &= ~((meta[:, 0] == 1) & (meta[:, 1] == 2) & (meta[:, 2] == 0))
    return trans[keep], meta[keep], frames[keep], gts


def _hr():
    rng = np.random.default_rng(1)
    return {(1, 1): rng.random(100) > 0.3, (2, 2): rng.random(100) > 0.5}


def _csr_pairs(plan):
    """{(person row, frame): [windows]} of the plan's window CSR"""
    ptr, idx, rows = plan.win_ptr.numpy(), plan.win_idx.numpy(), plan.row_ptr.numpy()
    out = {}
    for p in range(plan.n_persons):
        for f in range(int(plan.person_n[p])):
            e = rows[p] + f
            out[(p, f)] = idx[ptr[e]:ptr[e + 1]].tolist()
    return out


@pytest.mark.parametrize("case, num_transform", [(_base_case, 2), (_missing_clip_case, 1), (_ragged_case, 2), (_ragged_case, 1)])
def test_window_csr_holds_every_kept_pair_once(case, num_transform):
    trans, meta, frames, gts = case()
    gts = dict(gts)
    dropped_clip = sorted(gts)[-1] if case is _base_case else None
    if dropped_clip is not None:
        del gts[dropped_clip]                                 # windows of a clip without ground truth are dropped
    plan = E.ScorePlan(trans, meta, frames, gts, num_transform, device="cpu")
    assert plan.win_ptr.dtype == plan.win_idx.dtype == plan.row_ptr.dtype == plan.pc_ptr.dtype == torch.int32
    person_of = {tuple(k): p for p, k in enumerate(plan.person_keys.tolist())}
    want = {}
    for w in range(trans.shape[0]):
        t, (sc, cl, pe) = int(trans[w]), meta[w, :3].tolist()
        if t >= num_transform or (sc, cl) not in gts:
            continue
        for f in frames[w].tolist():
            want.setdefault((person_of[(t, sc, cl, pe)], f - 1), []).append(w)
    got = {k: v for k, v in _csr_pairs(plan).items() if v}
    assert got == want                                        # every kept (window, frame) once, ascending; dropped windows nowhere
    assert int(plan.win_ptr[-1]) == sum(len(v) for v in want.values()) == plan.win_idx.numel()
    assert plan.n_persons == len({k[0] for k in want}) == len(person_of)


def test_counts_segments_and_ground_truth_with_and_without_masks():
    trans, meta, frames, gts = _ragged_case()
    s = np.random.default_rng(0).random(trans.shape[0]) + 0.05
    for masks in (None, _hr()):
        plan = E.ScorePlan(trans, meta, frames, gts, 2, pad_size=4, hr_masks=masks, device="cpu")
        _, per_t_r, gt_r = RS.score_dataset(s, trans.numpy(), meta.numpy(), frames.numpy(), gts, 2, pad_size=4, hr_masks=masks)
        assert plan.n_clips == 4 and plan.n_persons == 2 * (3 * 4 - 1)          # person 0 of clip (1, 2) has no window left
        assert [tuple(k) for k in plan.person_keys.tolist()] == sorted({(int(t), *m[:3].tolist()) for t, m in zip(trans, meta)})
        lens = [int(masks[k].sum()) if masks and k in masks else 100 for k in sorted(gts)]
        bounds = np.cumsum([0] + lens)
        assert plan.segments.tolist() == [[int(a), int(b)] for a, b in zip(bounds[:-1], bounds[1:])]
        assert plan.F == bounds[-1] == per_t_r[0].shape[0]
        assert plan.gt.dtype == gt_r.dtype and np.array_equal(plan.gt, gt_r)
        assert np.array_equal(plan.gt_dev.numpy(), gt_r != 0)
        # every output position names its source (clip, frame)
        oc, of = plan.out_clip.numpy(), plan.out_frame.numpy()
        for c, k in enumerate(sorted(gts)):
            a, b = plan.segments[c]
            assert (oc[a:b] == c).all()
            assert np.array_equal(of[a:b], np.nonzero(masks[k])[0] if masks and k in masks else np.arange(100))
        # tiles cover every segment once, SP.TILE outputs each
        tiles = plan.tiles.numpy()
        assert sorted(tiles[:, 2].tolist()) == [s0 for a, b in plan.segments.tolist() for s0 in range(a, b, SP.TILE)]
        assert all(a <= s0 < b for a, b, s0 in tiles.tolist())
        # person CSR: the persons of (t, clip)
        pc = plan.pc_ptr.numpy()
        for t in range(2):
            for c, k in enumerate(sorted(gts)):
                rows = plan.person_keys[pc[t * 4 + c]:pc[t * 4 + c + 1]]
                assert (rows[:, 0] == t).all() and (rows[:, 1:3] == k).all() and rows.shape[0] == (2 if k == (1, 2) else 3)


def test_a_clip_without_persons_has_an_empty_person_list():
    trans, meta, frames, gts = _missing_clip_case()
    gts = dict(gts)
    gts[(9, 9)] = np.zeros(40, dtype=np.int64)
    plan = E.ScorePlan(trans, meta, frames, gts, 1, device="cpu")
    pc = plan.pc_ptr.numpy()
    assert plan.n_clips == 3 and pc[3] - pc[2] == 0 and plan.segments[2].tolist() == [160, 200]


def test_out_of_range_frame_number_raises_value_error():
    trans, meta, frames, gts = _base_case()
    for bad in (0, 91):
        fr = frames.clone()
        fr[17, 3] = bad
        with pytest.raises(ValueError, match="window 17"):
            E.ScorePlan(trans, meta, fr, gts, 2, device="cpu")
    fr = frames.clone()
    fr[17, 3] = 91
    gts1 = {k: v for k, v in gts.items() if k != tuple(meta[17, :2].tolist())}
    E.ScorePlan(trans, meta, fr, gts1, 2, device="cpu")       # a dropped window's frames are never used


def test_matches_only_the_tables_it_was_built_from():
    trans, meta, frames, gts = _base_case()
    plan = E.ScorePlan(trans, meta, frames, gts, 2, device="cpu")
    assert plan.matches(trans, meta, frames)
    assert plan.matches(trans.clone(), meta.clone().to(torch.int32), frames.clone().long())
    perm = torch.arange(trans.shape[0])
    perm[[5, 400]] = perm[[400, 5]]
    assert not plan.matches(trans[perm], meta[perm], frames[perm])
    fr = frames.clone()
    fr[100, 0] += 1
    assert not plan.matches(trans, meta, fr)
    assert not plan.matches(trans[:-1], meta[:-1], frames[:-1])
    assert plan.same_setting(gts, 2, -1, None) and not plan.same_setting(gts, 2, 4, None) and not plan.same_setting(gts, 1, -1, None)
    assert not plan.same_setting(gts, 2, -1, {(1, 1): np.arange(90) % 2 == 0})
    other = {k: (1 - v if k == (1, 1) else v) for k, v in gts.items()}
    assert not plan.same_setting(other, 2, -1, None)


def test_taps_are_scipys():
    taps = E.gaussian_taps()
    assert taps.shape == (121,) and taps.dtype == np.float64
    impulse = np.zeros(241)
    impulse[120] = 1.0
    response = gaussian_filter1d(impulse, 30)
    np.testing.assert_allclose(taps, response[120:], rtol=1e-15, atol=0)
    np.testing.assert_allclose(taps[::-1], response[:121], rtol=1e-15, atol=0)
    plan = E.ScorePlan(*_base_case()[:3], _base_case()[3], 2, device="cpu")
    assert plan.taps.dtype == torch.float64 and np.array_equal(plan.taps.numpy(), taps)


def test_constants_agree_with_the_library():
    lib = _lib.lib()
    assert lib.coskad_score_tile() == SP.TILE and lib.coskad_score_pad_row_max() == SP.PAD_ROW_MAX
    assert lib.coskad_score_auc_ws(1) == 1 and lib.coskad_score_auc_ws(SP.TILE + 1) == 2 and lib.coskad_score_auc_ws(0) == 0
    gts = {(1, 1): np.zeros(SP.PAD_ROW_MAX + 1, dtype=np.int64)}
    table = (torch.zeros(1, dtype=torch.int64), torch.tensor([[1, 1, 0, 0]]), torch.arange(1, 13, dtype=torch.int32)[None])
    E.ScorePlan(*table, gts, 1, device="cpu")
    with pytest.raises(ValueError, match="device_scoring: false"):
        E.ScorePlan(*table, gts, 1, pad_size=3, device="cpu")


def test_scoring_entry_points_refuse_bad_arguments_without_a_gpu():
    null = None
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    Err = _lib.CoskadHipError
    with pytest.raises(Err, match=r"\(-1\): score_person_frames: null pointer"):
        _lib.call("coskad_score_person_frames_f64", p, 1, p, null, p, 4, 4, null)
    with pytest.raises(Err, match=r"\(-1\): score_person_frames: n_scores=0 n_rows=4"):
        _lib.call("coskad_score_person_frames_f64", p, 0, p, p, p, 0, 4, null)
    with pytest.raises(Err, match=r"\(-1\): score_person_frames: n_scores=4 n_rows=-1"):
        _lib.call("coskad_score_person_frames_f64", p, 0, p, p, p, 4, -1, null)
    with pytest.raises(Err, match=r"\(-1\): score_pad: null pointer"):
        _lib.call("coskad_score_pad_f64", null, p, 3, 2, 50, null)
    with pytest.raises(Err, match=r"\(-1\): score_pad: n_persons=0"):
        _lib.call("coskad_score_pad_f64", p, p, 0, 2, 50, null)
    with pytest.raises(Err, match=r"\(-2\): score_pad: unsupported clip length 8193"):
        _lib.call("coskad_score_pad_f64", p, p, 3, 2, SP.PAD_ROW_MAX + 1, null)
    with pytest.raises(Err, match=r"\(-1\): score_clip_max: null pointer"):
        _lib.call("coskad_score_clip_max_f64", p, p, p, p, p, null, 2, 1, 8, null)
    with pytest.raises(Err, match=r"\(-1\): score_clip_max: n_clips=2 n_transform=0 F=8"):
        _lib.call("coskad_score_clip_max_f64", p, p, p, p, p, p, 2, 0, 8, null)
    with pytest.raises(Err, match=r"\(-1\): score_smooth: null pointer"):
        _lib.call("coskad_score_smooth_f64", p, p, null, 121, p, p, 1, 1, 8, null)
    with pytest.raises(Err, match=r"\(-1\): score_smooth: n_tiles=0"):
        _lib.call("coskad_score_smooth_f64", p, p, p, 121, p, p, 0, 1, 8, null)
    for n_taps in (120, 241):
        with pytest.raises(Err, match=rf"\(-2\): score_smooth: unsupported tap table of {n_taps} entries: the filter has 121 taps"):
            _lib.call("coskad_score_smooth_f64", p, p, p, n_taps, p, p, 1, 1, 8, null)
    with pytest.raises(Err, match=r"\(-1\): score_auc: null pointer"):
        _lib.call("coskad_score_auc_f64", p, p, p, p, null, 1, 8, null)
    with pytest.raises(Err, match=r"\(-1\): score_auc: F=0"):
        _lib.call("coskad_score_auc_f64", p, p, p, p, p, 1, 0, null)
    with pytest.raises(Err, match=r"\(-4\): score_auc: workspace of 1 elements, 2 needed"):
        _lib.call("coskad_score_auc_f64", p, p, p, p, p, 1, SP.TILE + 1, null)
    with pytest.raises(TypeError, match="argument 3: .*int32.*int64"):          # the tables are int32: bound from the header
        _lib.call("coskad_score_person_frames_f64", p, 0, torch.zeros(4, dtype=torch.int64), p, p, 4, 3, null)


def test_device_route_has_no_cpu_fallback():
    from coskad_amd import ops
    trans, meta, frames, gts = _base_case()
    plan = E.ScorePlan(trans, meta, frames, gts, 2, device="cpu")
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        E.score_dataset_device(torch.rand(trans.shape[0], dtype=torch.float64), plan)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.score_person_frames(torch.rand(8), plan.win_ptr, plan.win_idx)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.score_smooth(torch.rand(2, 8, dtype=torch.float64), plan.tiles, plan.taps)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.score_auc(torch.rand(8, dtype=torch.float64), torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int64))
