"""The frame-resident dataset (`dataset_resident: 'frames'`, coskad_amd.utils.dataset.PoseFramesRobust) on the CPU: one normalised
row per trajectory frame plus a row index per window must give the windows, items, metadata and frame ids of PoseDatasetRobust bit
for bit, and through it the reference's arrays of tests/golden/data_pipeline.npz (the CSV tree is rebuilt from the fixture as
tests/test_data_pipeline.py does)."""
import os
from argparse import Namespace
from collections import OrderedDict

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "data_pipeline.npz")
BASE = dict(num_transform=5, seg_len=12, vid_res=[1080, 720], num_coords=2)

# Settings beyond the golden's own.  On this tree (train trajectories of 40 / 9 / 30 / 25 frames, test 33 / 12 / 18) the window
# class yields windows for YIELDS on both splits and raises "no trajectory is long enough" for RAISES on both (checked on the CPU:
# seg_len 24 at stride 3 spans 70 frames).
YIELDS = [dict(kp18_format=True), dict(headless=True), dict(kp18_format=True, headless=True),
          dict(seg_len=8, seg_stride=1), dict(seg_len=8, seg_stride=3), dict(seg_len=24, seg_stride=1)]
RAISES = [dict(seg_len=24, seg_stride=3)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    g = np.load(GOLD)
    root = tmp_path_factory.mktemp("morais")
    for k in g.files:
        if not k.startswith("csv."):
            continue
        _, split, folder, person = k.split(".")
        d = root / ("training" if split == "train" else "testing") / "trajectories" / folder
        d.mkdir(parents=True, exist_ok=True)
        np.savetxt(d / f"{person}.csv", g[k], delimiter=",", fmt="%.6f")
    exp = str(tmp_path_factory.mktemp("exp"))
    from coskad_amd.utils.dataset import PoseDatasetRobust
    PoseDatasetRobust(str(root), split="train", exp_dir=exp, seg_stride=2, **BASE)      # pickles the scaler the test split loads
    return g, str(root), exp


def _order(meta):
    return np.lexsort((meta[:, 3], meta[:, 2], meta[:, 1], meta[:, 0]))


def _pair(root, exp, split, **over):
    from coskad_amd.utils.dataset import PoseDatasetRobust, PoseFramesRobust
    kw = dict(BASE, exp_dir=exp, seg_stride=2 if split == "train" else 1)
    kw.update(over)
    return PoseDatasetRobust(root, split=split, **kw), PoseFramesRobust(root, split=split, **kw)


def _assert_same(win, fr):
    """every window, item, metadata row and frame-id row, in the same order, bit for bit"""
    assert (fr.num_samples, fr.C, fr.T, fr.V) == (win.num_samples, win.C, win.T, win.V) and len(fr) == len(win)
    assert fr.num_transform == win.num_transform
    np.testing.assert_array_equal(fr.trans_mats, win.trans_mats)
    np.testing.assert_array_equal(fr.scaler.center_, win.scaler.center_)
    np.testing.assert_array_equal(fr.scaler.scale_, win.scaler.scale_)
    assert fr.frame_xy.dtype == np.float32 and fr.frame_xy.shape == (len(fr.frame_id), 2, win.V)
    assert fr.frame_id.dtype == np.int32 and fr.win_row.dtype == np.int32 and fr.win_row.shape == (win.num_samples,)
    assert fr.metadata is fr.segs_meta
    np.testing.assert_array_equal(fr.segs_meta, win.segs_meta)
    assert fr.segs_ids.shape == win.segs_ids.shape
    np.testing.assert_array_equal(np.asarray(fr.segs_ids), win.segs_ids)
    for s in range(win.num_samples):
        w = fr.window(s)
        assert w.dtype == np.float32 and np.array_equal(w, win.segs_data_np[s]), s
        assert np.array_equal(fr.segs_ids[s], win.segs_ids[s])
    for i in range(len(win)):
        a, b = win[i], fr[i]
        assert a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]), i
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), i


@pytest.mark.parametrize("split", ["train", "test"])
def test_golden_settings_match_the_window_class_and_the_reference(tree, split):
    g, root, exp = tree
    win, fr = _pair(root, exp, split)
    _assert_same(win, fr)
    # ... and the reference's own arrays, after the metadata ordering of tests/test_data_pipeline.py
    ref_meta, ref_ids, ref_data = g[f"{split}.meta"], g[f"{split}.ids"], g[f"{split}.data"]
    assert len(fr) == int(g[f"{split}.len"])
    a, b = _order(fr.segs_meta), _order(ref_meta)
    np.testing.assert_array_equal(fr.segs_meta[a], ref_meta[b])
    np.testing.assert_array_equal(fr.segs_ids[a], ref_ids[b])
    np.testing.assert_array_equal(np.stack([fr.window(s) for s in a]), ref_data[b])
    n = fr.num_samples
    for k, ref_index in enumerate(g[f"{split}.item_index"]):
        t = int(ref_index) // n
        m = g[f"{split}.item_meta"][k]
        s = int(np.flatnonzero((fr.segs_meta == m).all(1))[0])
        data, tt, meta, ids = fr[t * n + s]
        assert tt == t == int(g[f"{split}.item_trans"][k]) and data.shape == (2, 12, 17)
        np.testing.assert_array_equal(meta, m)
        np.testing.assert_array_equal(ids, g[f"{split}.item_ids"][k])
        np.testing.assert_allclose(data, g[f"{split}.item_data"][k], rtol=0, atol=1e-7)      # the existing item test's bound


@pytest.mark.parametrize("split", ["train", "test"])
@pytest.mark.parametrize("over", YIELDS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_other_layouts_lengths_and_strides(tree, split, over):
    _, root, exp = tree
    win, fr = _pair(root, exp, split, **over)
    assert win.num_samples >= 1
    _assert_same(win, fr)


@pytest.mark.parametrize("split", ["train", "test"])
@pytest.mark.parametrize("over", RAISES, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_no_window_raises_as_the_window_class_does(tree, split, over):
    from coskad_amd.utils.dataset import PoseDatasetRobust, PoseFramesRobust
    _, root, exp = tree
    for cls in (PoseDatasetRobust, PoseFramesRobust):
        with pytest.raises(ValueError, match="no trajectory is long enough"):
            cls(root, split=split, exp_dir=exp, **dict(BASE, **over))


def test_segs_ids_indexes_like_the_array(tree):
    _, root, exp = tree
    win, fr = _pair(root, exp, "test")
    mask = win.segs_meta[:, 2] == win.segs_meta[0, 2]
    for key in (3, -1, slice(2, 9, 3), mask, np.array([5, 0, 5]), (mask, 0), (slice(None), -1), (4, 2)):
        np.testing.assert_array_equal(fr.segs_ids[key], win.segs_ids[key])
    assert int(fr.segs_ids[mask].max()) == int(win.segs_ids[mask].max()) and len(fr.segs_ids) == len(win.segs_ids)


def test_no_window_sized_float_table(tree):
    """seg_len 24 at stride 1: 24 float rows per window against one per frame.  Only shapes and dtypes are looked at: every float
    array the object holds has one row per FRAME, none has a window axis."""
    _, root, exp = tree
    _, fr = _pair(root, exp, "train", seg_len=24, seg_stride=1)
    F, N = len(fr.frame_id), fr.num_samples
    assert N * 24 > 4 * F                                         # the window table would be several times the frame table
    floats = {k: v for k, v in vars(fr).items() if isinstance(v, np.ndarray) and v.dtype.kind == "f"}
    assert set(floats) == {"frame_xy", "trans_mats"}
    assert fr.frame_xy.shape == (F, 2, 17) and fr.frame_xy.dtype == np.float32
    assert fr.trans_mats.shape == (5, 3, 3)
    assert fr.win_row.shape == (N,) and fr.frame_id.shape == (F,) and fr.segs_meta.shape == (N, 4)
    assert not isinstance(fr.segs_ids, np.ndarray) and fr.segs_ids.shape == (N, 24)
    assert not hasattr(fr, "segs_data_np")


def _write_traj(root, sub, folder, person, n, first=0):
    d = root / sub / "trajectories" / folder
    d.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(n)
    rows = np.concatenate([np.arange(first, first + n)[:, None], rng.uniform(50, 600, (n, 34))], 1)
    np.savetxt(d / f"{person}.csv", rows, delimiter=",", fmt="%.6f")


def test_one_window_trajectory_and_overrunning_rows(tmp_path):
    from coskad_amd.utils.dataset import PoseDatasetRobust, PoseFramesRobust, check_window_rows
    _write_traj(tmp_path, "training", "01-0001", "0001", 12, first=5)        # exactly one window
    _write_traj(tmp_path, "training", "01-0001", "0002", 3)                  # too short: dropped
    kw = dict(BASE, exp_dir=str(tmp_path / "exp"))
    fr = PoseFramesRobust(str(tmp_path), split="train", **kw)
    assert fr.num_samples == 1 and fr.win_row.tolist() == [0] and len(fr.frame_id) == 12
    assert fr.segs_meta.tolist() == [[1, 1, 1, 5]] and fr.segs_ids[0].tolist() == list(range(5, 17))
    _assert_same(PoseDatasetRobust(str(tmp_path), split="train", **kw), fr)
    # two trajectories of 12 and 20 rows, windows of 12 frames
    ptr = np.array([0, 12, 32])
    check_window_rows(np.array([0, 12, 20]), ptr, 12, 1)
    for bad in ([1], [0, 21], [-1], [32], [0, 12, 40]):
        with pytest.raises(ValueError, match="leaves its trajectory"):
            check_window_rows(np.array(bad), ptr, 12, 1)
    with pytest.raises(ValueError, match="leaves its trajectory"):
        check_window_rows(np.array([12]), ptr, 12, 2)                         # 12 + 11 * 2 = 34: past the second trajectory
    check_window_rows(np.array([12]), ptr, 10, 2)                             # 12 + 9 * 2 = 30: inside
    with pytest.raises(ValueError, match="2\\^31"):
        check_window_rows(np.array([0]), np.array([0, 2 ** 31]), 12, 1)
    check_window_rows(np.array([0]), np.array([0, 2 ** 31 - 1]), 12, 1)
    with pytest.raises(ValueError, match="no trajectory is long enough"):
        check_window_rows(np.array([], dtype=np.int64), ptr, 12, 1)


def test_dataset_resident_selects_the_class(tree, monkeypatch):
    """unset or 'windows': today's classes; 'frames': the frame classes; anything else raises (no device is touched: to_device is
    replaced by a marker)"""
    from coskad_amd.utils import dataset as D
    _, root, exp = tree
    monkeypatch.setattr(D.PoseDatasetRobust, "to_device", lambda self, device="cuda": ("windows", self))
    monkeypatch.setattr(D.PoseFramesRobust, "to_device", lambda self, device="cuda": ("frames", self))
    base = dict(num_coords=2, dataset_path_to_robust=root, dataset_seg_len=12, dataset_seg_stride=2, dataset_exp_dir=exp,
                dataset_batch_size=16, dataset_num_transform=5, seed=0)
    for extra, cls, tag in (({}, D.PoseDatasetRobust, "windows"), ({"dataset_resident": "windows"}, D.PoseDatasetRobust, "windows"),
                            ({"dataset_resident": "frames"}, D.PoseFramesRobust, "frames")):
        ds, loader = D.get_dataset_and_loader(Namespace(**base, **extra), split="train")
        assert type(ds) is cls and loader.w == (tag, ds) and ds.seg_len == 12
    ds, _ = D.get_dataset_and_loader(Namespace(**base, dataset_resident="frames"), split="test")
    assert type(ds) is D.PoseFramesRobust and ds.step == 1                  # the stride is the train split's alone
    for bad in ("frame", "Frames", "", None, 1):
        with pytest.raises(ValueError, match="dataset_resident"):
            D.get_dataset_and_loader(Namespace(**base, dataset_resident=bad), split="train")
