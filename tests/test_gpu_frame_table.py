"""The frame-resident device table (`dataset_resident: 'frames'`): coskad_gather_frames_f32 (csrc/data.hip) forms each batch from one
normalised row per trajectory frame.  It must give the bits of the window table's coskad_gather_transform_f32 on the golden tree, the
bits of a float64 restatement on synthetic tables, zero clips for the inputs it handles instead of reading out of bounds, the same
DeviceLoader batches, and the same training run."""
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "data_pipeline.npz")
KW = dict(num_transform=5, seg_len=12, vid_res=[1080, 720], num_coords=2)


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
    shutil.copytree(root / "testing", root / "validating")
    return str(root), str(tmp_path_factory.mktemp("exp"))


@pytest.fixture(scope="module")
def tables(tree):
    """{split: (DeviceWindows, FrameWindows)} at the golden's settings (train stride 2, test stride 1)"""
    from coskad_amd.utils.dataset import PoseDatasetRobust, PoseFramesRobust
    root, exp = tree
    out = {}
    for split, stride in (("train", 2), ("test", 1)):
        w = PoseDatasetRobust(root, split=split, exp_dir=exp, seg_stride=stride, **KW)
        f = PoseFramesRobust(root, split=split, exp_dir=exp, seg_stride=stride, **KW)
        out[split] = (w.to_device("cuda"), f.to_device("cuda"))
    return out


@pytest.mark.parametrize("split", ["train", "test"])
def test_golden_tree_gathers_the_window_tables_bits(tables, split):
    w, f = tables[split]
    assert (f.N, f.T, f.V) == (w.N, w.T, w.V) and f.ds.num_samples == f.N
    assert f.fxy.is_cuda and f.fxy.dtype == torch.float32 and tuple(f.fxy.shape) == (len(f.ds.frame_id), 2, 17)
    assert f.win_row_dev.is_cuda and f.win_row_dev.dtype == torch.int32 and not f.win_row.is_cuda and not f.frame_id.is_cuda
    index = torch.arange(len(w.ds))
    a, b = w.gather(index), f.gather(index)
    assert tuple(b.shape) == (len(w.ds), 2, 12, 17) and torch.equal(a, b)
    assert torch.equal(w.meta, f.meta) and torch.equal(w.frames[index % w.N], f.frames[index % f.N])
    assert f.frames[index % f.N].dtype == torch.int32


def test_num_coords_other_than_two_is_refused(tree):
    from coskad_amd.utils.dataset import PoseFramesRobust
    root, exp = tree
    ds = PoseFramesRobust(root, split="test", exp_dir=exp, **dict(KW, num_coords=3))
    assert ds[0][0].shape == (3, 12, 17)
    with pytest.raises(ValueError, match="num_coords = 2"):
        ds.to_device("cuda")


# ---- synthetic tables against a float64 restatement --------------------------------------------------------------------------------

def _table(T, V, step, seed):
    """three trajectories of different lengths, every valid window start; float32 rows"""
    gen = np.random.default_rng(seed)
    span = (T - 1) * step
    lengths = [span + 1, span + 9, span + 4]                       # one window, nine windows, four windows
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    win_row = np.concatenate([o + np.arange(n - span) for o, n in zip(ptr, lengths)]).astype(np.int32)
    fxy = gen.standard_normal((int(ptr[-1]), 2, V)).astype(np.float32)
    mats = gen.standard_normal((5, 3, 3)).astype(np.float32)
    return fxy, win_row, mats


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _restated(fxy, win_row, mats, index, T, step):
    """(M[c][0] x + M[c][1] y) + M[c][2] in float64 with every operation's result rounded to float32.  A float64 product of two
    float32 values is exact, and a float64 sum rounded to float32 is the correctly rounded float32 sum (53 >= 2 * 24 + 2 bits: the
    double rounding is innocuous), so this reproduces the kernel's fp32 association and the comparison is EXACT, not within an ulp.
    An index outside [0, N ntrans) or a window with a row outside [0, F) is a zero clip."""
    F, _, V = fxy.shape
    N = len(win_row)
    f, m = fxy.astype(np.float64), mats.astype(np.float64)
    out = np.zeros((len(index), 2, T, V), np.float64)
    for b, i in enumerate(index):
        i = int(i)
        if i < 0 or i // N >= len(mats):
            continue
        s, tr = i % N, i // N
        r0 = int(win_row[s])
        if r0 < 0 or r0 + (T - 1) * step >= F:
            continue
        rows = r0 + step * np.arange(T)
        x, y = f[rows, 0], f[rows, 1]                               # [T, V]
        for c in range(2):
            out[b, c] = _f32(_f32(_f32(x * m[tr, c, 0]) + _f32(y * m[tr, c, 1])) + m[tr, c, 2])
    return out.astype(np.float32)


SHAPES = [(7, 17, 1), (12, 14, 3), (8, 18, 2), (24, 17, 1)]       # scalar path (119 positions); step 3; step 2; 4-groups straddling frames


@pytest.mark.parametrize("B", [1, 67])
@pytest.mark.parametrize("T,V,step", SHAPES)
def test_synthetic_table_equals_the_float64_restatement(T, V, step, B):
    """exact equality (see _restated).  B = 67 leaves the last block ragged in both kernels and holds the first and the last item;
    B = 1 is the last item: last window of the last trajectory (its last row is the table's last), last transform."""
    from coskad_amd import ops
    fxy, win_row, mats = _table(T, V, step, seed=T * 100 + V)
    N, last = len(win_row), len(win_row) * 5 - 1
    if B == 1:
        idx = [last]
    else:
        idx = np.random.default_rng(B).integers(0, last + 1, B).tolist()
        idx[0], idx[-1] = 0, last
    got = ops.gather_frames(torch.from_numpy(fxy).cuda(), torch.from_numpy(win_row).cuda(), torch.from_numpy(mats).cuda(),
                            torch.tensor(idx, dtype=torch.int64).cuda(), T, V, step)
    assert tuple(got.shape) == (B, 2, T, V) and got.dtype == torch.float32
    want = _restated(fxy, win_row, mats, idx, T, step)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert all(got[b].any() for b in range(B))


@pytest.mark.parametrize("T,V,step", [(7, 17, 1), (24, 17, 1), (12, 14, 3)])
def test_handled_out_of_range_inputs_give_zero_clips(T, V, step):
    """index -1 and N ntrans + 5, and win_row entries that would leave the table (one row too far, negative, far beyond): zero
    clips, the neighbours right, the guard behind `out` untouched.  The kernel checks each of them before it forms an address."""
    from coskad_amd import _lib, ops
    fxy, win_row, mats = _table(T, V, step, seed=7)
    F, N = fxy.shape[0], len(win_row)
    win_row = win_row.copy()
    bad_rows = {2: F - (T - 1) * step, 5: -3, 9: F + 100}          # window -> first row; F - span is the first that overruns
    for s, r in bad_rows.items():
        win_row[s] = r
    idx = [0, -1, 1, 2, 3, N * 5 + 5, N * 5 - 1, N + 5, 4, 2 * N + 9, 8, 3 * N + 2, -N * 5 - 1, 6]
    zero = [b for b, i in enumerate(idx) if i < 0 or i >= N * 5 or i % N in bad_rows]
    assert len(zero) == 7
    dev = [torch.from_numpy(a).cuda() for a in (fxy, win_row, mats)]
    index = torch.tensor(idx, dtype=torch.int64).cuda()
    want = _restated(fxy, win_row, mats, idx, T, step)
    got = ops.gather_frames(dev[0], dev[1], dev[2], index, T, V, step).cpu().numpy()
    assert np.array_equal(got, want)
    for b in range(len(idx)):
        assert got[b].any() == (b not in zero), b
    # the same call into a buffer with guard elements behind `out`
    n, guard = len(idx) * 2 * T * V, 256
    buf = torch.full((n + guard,), 12345.0, device="cuda")
    _lib.call("coskad_gather_frames_f32", dev[0], dev[1], index, dev[2], buf, len(idx), N, F, 5, T, V, step,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf[:n].cpu().numpy().reshape(want.shape), want)
    assert bool((buf[n:] == 12345.0).all())


def test_argument_checks_come_before_the_launch():
    from coskad_amd import _lib
    fxy, win_row, mats = (torch.from_numpy(a).cuda() for a in _table(8, 18, 2, seed=1))
    index, out = torch.zeros(1, dtype=torch.int64).cuda(), torch.full((2 * 8 * 18,), 7.0, device="cuda")
    good = dict(B=1, N=win_row.numel(), F=fxy.shape[0], ntrans=5, T=8, V=18, step=2)
    s = torch.cuda.current_stream().cuda_stream
    for k, v in (("B", 0), ("N", 0), ("F", 0), ("F", 2 ** 31), ("ntrans", 0), ("T", 0), ("V", -1), ("step", 0)):
        a = dict(good, **{k: v})
        with pytest.raises(_lib.CoskadHipError, match="gather_frames"):
            _lib.call("coskad_gather_frames_f32", fxy, win_row, index, mats, out, a["B"], a["N"], a["F"], a["ntrans"], a["T"], a["V"],
                      a["step"], s)
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        _lib.call("coskad_gather_frames_f32", fxy, None, index, mats, out, 1, good["N"], good["F"], 5, 8, 18, 2, s)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the loader and a training run ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rank", [0, 1])
def test_device_loader_batches_are_the_same(tables, rank):
    from coskad_amd.utils.dataset import DeviceLoader
    w, f = tables["train"]
    la = DeviceLoader(w, 16, shuffle=True, seed=3, rank=rank, world=2)
    lb = DeviceLoader(f, 16, shuffle=True, seed=3, rank=rank, world=2)
    assert len(la) == len(lb)
    for _ in range(2):                                               # two epochs: the permutation changes with the epoch
        a, b = list(la), list(lb)
        assert len(a) == len(b) == len(la)
        for (xa, ta, ma, fa), (xb, tb, mb, fb) in zip(a, b):
            assert xb.is_cuda and torch.equal(xa, xb) and torch.equal(ta, tb) and torch.equal(ma, mb) and torch.equal(fa, fb)
            assert fa.dtype == fb.dtype and ma.dtype == mb.dtype


def _fit(root, exp_dir, resident):
    from coskad_amd.lit import LitEncoder, Trainer
    from coskad_amd.utils.dataset import get_dataset_and_loader
    args = Namespace(num_coords=2, h_dim=16, latent_dim=8, dataset_seg_len=12, dropout=0, channels=[16, 8, 16],
                     projector="linear", encoder_type="STS_GCN", hyperbolic=False, static_center=False,
                     center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6, dataset_batch_size=32, dataset_num_transform=5,
                     dataset_headless=False, dataset_kp18_format=False, smoothing=5, dataset_choice="UBnormal",
                     validation=True, dataset_path_to_robust=root, dataset_seg_stride=2, dataset_vid_res=[1080, 720],
                     dataset_normalize_pose=True, dataset_exp_dir=str(exp_dir), seed=0, debug=False)
    if resident is not None:
        args.dataset_resident = resident
    torch.manual_seed(0)
    ds, train_loader, vds, val_loader = get_dataset_and_loader(args, split="train", validation=True)
    lit = LitEncoder(args).cuda()
    gts = {}
    for sc, cl in {(int(m[0]), int(m[1])) for m in vds.segs_meta}:
        n = int(vds.segs_ids[(vds.segs_meta[:, 0] == sc) & (vds.segs_meta[:, 1] == cl)].max()) + 1
        gt = np.zeros(n, dtype=np.int64)
        gt[n // 2: n // 2 + 5] = 1
        gts[(sc, cl)] = gt
    lit.gts = gts
    tr = Trainer(max_epochs=2, ckpt_dir=str(exp_dir / "ck"))
    tr.fit(lit, lambda: train_loader, lambda: val_loader)
    return type(ds).__name__, [(h["loss"], h["validation_auc"]) for h in tr.history]


def test_fit_from_frames_equals_fit_from_windows(tree, tmp_path):
    """tests/test_data_pipeline.py::test_fit_and_score_from_morais_tree twice from one seed.  The batches are bit-identical and the
    step is deterministic, so the histories (loss, validation_auc) are EQUAL, not close."""
    root, _ = tree
    (tmp_path / "f").mkdir(); (tmp_path / "w").mkdir()
    name_f, hist_f = _fit(root, tmp_path / "f", "frames")
    name_w, hist_w = _fit(root, tmp_path / "w", "windows")
    print("frames ", hist_f)
    print("windows", hist_w)
    assert (name_f, name_w) == ("PoseFramesRobust", "PoseDatasetRobust")
    assert len(hist_f) == 2 and all(np.isfinite(h[0]) and 0.0 <= h[1] <= 1.0 for h in hist_f)
    assert hist_f == hist_w
