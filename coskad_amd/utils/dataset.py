"""Data pipeline of the reference's `normalization_strategy: 'robust'` path, restated array-wise.

Reference flow (utils/dataset.py:204-327 -> utils/get_robust_data.py:24-185 -> utils/data.py, utils/preprocessing.py,
utils/dataset_utils.py):  Morais-format CSV trajectories `<root>/{training,validating,testing}/trajectories/<SS-CCCC>/
<PPPP>.csv` (rows `frame, x1, y1, ..., x17, y17`, zeros = missing joint) -> drop trajectories shorter than a window ->
bounding-box-centred coordinates per frame -> sliding windows -> RobustScaler (quantiles 10/90, zeros ignored, fitted on
the train split and pickled as `<exp_dir>/local_robust.pickle`) -> [N, 3, T, V] (x, y, 1) -> optional 18-keypoint /
headless layouts -> one of 5 affine `PoseTransform`s per item.

MI355X-first design: the window table is small next to 288 GB of HBM (one million windows = 1.6 GB), so `DeviceLoader`
keeps it RESIDENT on the GPU and forms each batch with one gather + affine kernel (`coskad_gather_transform_f32`):
no per-step host->device traffic, no DataLoader workers.  The numpy `__getitem__` of the reference surface is kept for
parity tests and for CPU-side consumers.

`dataset_resident: 'frames'` (PoseFramesRobust / FrameWindows) keeps one normalised row per trajectory FRAME instead: overlapping
windows share their frames, a window is a row index, and `coskad_gather_frames_f32` forms the batch from the frames -- the same bits
from 1 / T of the memory (at stride 1).  `num_coords = 2` and this robust path only.

Pinned by tests/golden/data_pipeline.npz (generated from the reference by oracle/make_golden_data.py).
"""
from __future__ import annotations

import math
import os
import pickle
from collections import OrderedDict
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

N_KP = 17


# ---- trajectories -------------------------------------------------------------------------------------------
def load_trajectories(trajectories_path: str, debug: bool = False, split: str = 'train') -> "OrderedDict[str, Tuple[np.ndarray, np.ndarray]]":
    """utils/data.py:218-235.  id `<SS-CCCC>_<PPPP>` -> (frames int32 [n], coordinates float32 [n, 34]).
    Folders and files are visited in sorted order (the reference uses os.listdir order, which is unspecified)."""
    out: "OrderedDict[str, Tuple[np.ndarray, np.ndarray]]" = OrderedDict()
    folders = sorted(os.listdir(trajectories_path))
    if debug and split == 'train':
        folders = folders[:5]
    for folder in folders:
        for name in sorted(os.listdir(os.path.join(trajectories_path, folder))):
            arr = np.loadtxt(os.path.join(trajectories_path, folder, name), dtype=np.float32, delimiter=',', ndmin=2)
            out[folder + '_' + name.split('.')[0]] = (arr[:, 0].astype(np.int32), arr[:, 1:])
    return out


def bbox_centre_coordinates(coords: np.ndarray, video_resolution: Sequence[float]) -> np.ndarray:
    """All frames of a trajectory at once: utils/data.py:9-43 (`compute_bounding_box`: min/max over the non-zero x
    resp. y, 10 % margin, clipped to the frame, rounded half-to-even) and :159-181 (`_from_image_to_centre_bounding_box`:
    missing joints -> centre, subtract the centre, divide by the box size; frames without any joint stay zero)."""
    c = np.asarray(coords, dtype=np.float32)
    n = c.shape[0]
    width, height = np.asarray(video_resolution, dtype=np.float32)
    x, y = c[:, 0::2], c[:, 1::2]
    xm, ym = x != 0, y != 0
    some = xm.any(1) | ym.any(1)                       # `any(kps)`
    boxed = xm.any(1) & ym.any(1)                      # else np.min of an empty array -> the (0, 0, 0, 0) box
    inf = np.float32(np.inf)
    left = np.where(xm, x, inf).min(1)
    right = np.where(xm, x, -inf).max(1)
    top = np.where(ym, y, inf).min(1)
    bottom = np.where(ym, y, -inf).max(1)
    with np.errstate(invalid='ignore', over='ignore'):
        ew = np.float32(0.1) * (right - left + np.float32(1))
        eh = np.float32(0.1) * (bottom - top + np.float32(1))
        l_ = np.rint(np.clip(left - ew, np.float32(0), width - np.float32(1)))
        r_ = np.rint(np.clip(right + ew, np.float32(0), width - np.float32(1)))
        t_ = np.rint(np.clip(top - eh, np.float32(0), height - np.float32(1)))
        b_ = np.rint(np.clip(bottom + eh, np.float32(0), height - np.float32(1)))
    l_, r_, t_, b_ = (np.where(boxed, v, 0).astype(np.float32) for v in (l_, r_, t_, b_))
    cx, cy = (l_ + r_) / np.float32(2), (t_ + b_) / np.float32(2)      # integers / 2: exact in float32
    w, h = r_ - l_, b_ - t_
    xs = np.where(xm, x, cx[:, None]) - cx[:, None]
    ys = np.where(ym, y, cy[:, None]) - cy[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        xs = np.where(w[:, None] != 0, xs / w[:, None], np.float32(0))
        ys = np.where(h[:, None] != 0, ys / h[:, None], np.float32(0))
    out = np.empty((n, 2 * x.shape[1]), dtype=np.float32)
    out[:, 0::2], out[:, 1::2] = xs, ys
    out[~some] = c[~some]
    return out


def build_windows(trajs: "OrderedDict[str, Tuple[np.ndarray, np.ndarray]]", seg_len: int, gap: int):
    """utils/preprocessing.py:244-313: every start, `seg_len` frames `gap + 1` apart.
    -> X [N, seg_len, D] f32, meta [N, 4] (scene, clip, person, first frame id), ids [N, seg_len] (frame ids)."""
    total = seg_len + gap * (seg_len - 1)
    Xs, metas, ids = [], [], []
    for tid, (frames, coords) in trajs.items():
        n = len(frames)
        starts = np.arange(0, n - total + 1)
        if starts.size == 0:
            continue
        idx = starts[:, None] + (gap + 1) * np.arange(seg_len)[None, :]
        Xs.append(coords[idx])
        scene, clip = (int(v) for v in tid.split('_')[0].split('-'))
        person = int(tid.split('_')[1])
        metas.append(np.stack([np.full(starts.size, scene), np.full(starts.size, clip), np.full(starts.size, person),
                               frames[starts]], 1).astype(np.int64))
        ids.append(frames[idx].astype(np.int64))
    if not Xs:
        raise ValueError("no trajectory is long enough for one window")
    return np.concatenate(Xs, 0), np.concatenate(metas, 0), np.concatenate(ids, 0)


def scale_robust(X: np.ndarray, scaler=None):
    """utils/data.py:361-370: zeros are missing values; RobustScaler(quantile_range=(10, 90)); missing -> 0."""
    from sklearn.preprocessing import RobustScaler
    shape = X.shape
    Xn = np.where(X == 0.0, np.nan, X).reshape(-1, shape[-1])
    if scaler is None:
        scaler = RobustScaler(quantile_range=(10.0, 90.0))
        scaler.fit(Xn)
    Xs = scaler.transform(Xn)
    return np.where(np.isnan(Xs), 0.0, Xs).reshape(shape), scaler


def keypoints17_to_coco18(kps: np.ndarray) -> np.ndarray:
    """utils/dataset_utils.py:7-19: neck = mean of the shoulders (5, 6), then the OpenPose order."""
    neck = 0.5 * (kps[..., 5, :] + kps[..., 6, :])
    kp = np.concatenate([kps, neck[..., None, :]], axis=-2)
    return kp[..., np.array([0, 17, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3]), :]


# ---- the 5 affine transforms (utils/dataset_utils.py:255-310) ---------------------------------------------------
def aff_trans_mat(sx=1.0, sy=1.0, tx=0.0, ty=0.0, rot=0.0, flip=False) -> np.ndarray:
    """flip . rot . [scale | translate]  as float32 3x3 (each factor rounded to float32 first, like the torch original)."""
    c, s = math.cos(math.radians(rot)), math.sin(math.radians(rot))
    f = np.eye(3, dtype=np.float32)
    if flip:
        f[0, 0] = -1.0
    ts = np.array([[sx, 0, tx], [0, sy, ty], [0, 0, 1]], dtype=np.float32)
    r = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    return (f @ (r @ ts)).astype(np.float32)


AE_TRANS_MATS = np.stack([aff_trans_mat(rot=0, flip=False), aff_trans_mat(rot=0, flip=True),
                          aff_trans_mat(rot=90, flip=False), aff_trans_mat(rot=90, flip=True),
                          aff_trans_mat(rot=45, flip=False)])


def apply_pose_transform(pose: np.ndarray, mat: np.ndarray) -> np.ndarray:
    """pose [3, T, V] = (x, y, conf): transform (x, y, 1), keep conf (utils/dataset_utils.py:272-286)."""
    hom = np.concatenate([pose[:2], np.ones_like(pose[2:3])], 0)
    out = np.einsum('ktv,ck->ctv', hom, mat)
    return np.concatenate([out[:2], pose[2:3]], 0)


# ---- dataset ----------------------------------------------------------------------------------------------------------
def robust_front_end(path_to_robust_data: str, split: str, exp_dir: str, seg_len: int, seg_stride: int,
                     vid_res: Sequence[int], normalize_pose: bool, debug: bool, scaler):
    """What both residencies share: the split's trajectories without those shorter than one window, in bounding-box-centred
    coordinates, and the RobustScaler (given; or fitted on the train split's frames and pickled as <exp_dir>/local_robust.pickle;
    or loaded from there).  -> (trajs, scaler); scaler stays as given where normalize_pose is off."""
    sub = 'training' if 'train' in split else ('testing' if 'test' in split else 'validating')
    trajs = load_trajectories(os.path.join(path_to_robust_data, sub, 'trajectories'), debug=debug, split=split)
    total = seg_len + (seg_stride - 1) * (seg_len - 1)
    trajs = OrderedDict((k, v) for k, v in trajs.items() if len(v[0]) >= total)          # remove_short_trajectories
    if not trajs:
        raise ValueError("no trajectory is long enough for one window")
    res = np.asarray(vid_res, dtype=np.float32)
    trajs = OrderedDict((k, (f, bbox_centre_coordinates(c, res))) for k, (f, c) in trajs.items())
    if normalize_pose and scaler is None:
        path = os.path.join(exp_dir, 'local_robust.pickle')
        if split == 'train':
            _, scaler = scale_robust(np.vstack([c for _, c in trajs.values()]))
            if exp_dir:
                os.makedirs(exp_dir, exist_ok=True)
                with open(path, 'wb') as f:
                    pickle.dump(scaler, f)
        else:
            with open(path, 'rb') as f:
                scaler = pickle.load(f)
    return trajs, scaler


def pose_layout(X: np.ndarray, kp18_format: bool, headless: bool) -> np.ndarray:
    """[..., 34] (x1, y1, ...) -> float64 [..., V, 3] of (x, y, 1) triples: V = 17, 18 with `kp18_format`, 14 with `headless`.
    Every op is element-wise or per frame, so frames and windows of frames get the same values."""
    kp = X.reshape(*X.shape[:-1], N_KP, 2)
    data = np.empty((*kp.shape[:-1], 3))
    data[..., :2], data[..., 2] = kp, 1.0
    if kp18_format:
        data = keypoints17_to_coco18(data)
    if headless:
        data = data[..., :14, :]
    return data


class PoseDatasetRobust:
    """Array-wise restatement of utils/dataset.py::PoseDatasetRobust (local features only: `include_global=False`).
    Attributes follow the reference: segs_data_np [N, 3, T, V] f32, segs_meta [N, 4], segs_ids [N, T], num_samples,
    num_transform; item `i` = transform `i // N` of window `i % N` -> [data [num_coords, T, V], trans, meta, ids]."""

    def __init__(self, path_to_robust_data: str, split: str = 'train', exp_dir: str = '', num_transform: int = 5,
                 seg_len: int = 12, seg_stride: int = 1, vid_res: Sequence[int] = (1080, 720), num_coords: int = 2,
                 normalize_pose: bool = True, kp18_format: bool = False, headless: bool = False, debug: bool = False,
                 scaler=None) -> None:
        self.split, self.num_coords, self.seg_len = split, num_coords, seg_len
        self.num_transform = max(1, int(num_transform))
        self.trans_mats = AE_TRANS_MATS[:self.num_transform] if num_transform > 0 else AE_TRANS_MATS[:1]
        trajs, self.scaler = robust_front_end(path_to_robust_data, split, exp_dir, seg_len, seg_stride, vid_res,
                                              normalize_pose, debug, scaler)
        X, meta, ids = build_windows(trajs, seg_len, seg_stride - 1)
        if normalize_pose:
            X, _ = scale_robust(X, self.scaler)
        data = pose_layout(X, kp18_format, headless)
        self.segs_data_np = np.transpose(data, (0, 3, 1, 2)).astype(np.float32)
        self.segs_meta, self.segs_ids = meta, ids
        self.metadata = self.segs_meta
        self.num_samples, self.C, self.T, self.V = self.segs_data_np.shape

    def __len__(self) -> int:
        return self.num_transform * self.num_samples

    def __getitem__(self, index: int):
        s, t = index % self.num_samples, index // self.num_samples
        data = apply_pose_transform(self.segs_data_np[s], self.trans_mats[t])[:self.num_coords]
        return [data, t, self.segs_meta[s], self.segs_ids[s]]

    def to_device(self, device="cuda") -> "DeviceWindows":
        return DeviceWindows(self, device)


class DeviceWindows:
    """The window table resident in HBM: xy [N, 2, T*V] f32 (conf is the constant 1 of the robust path) and the
    transform matrices; `gather(index)` = one HIP kernel producing the batch [B, 2, T, V] for dataset indices."""

    def __init__(self, ds: PoseDatasetRobust, device="cuda") -> None:
        if ds.num_coords != 2:
            raise ValueError("the device loader serves the (x, y) layout (num_coords = 2)")
        self.ds = ds
        self.N, self.T, self.V = ds.num_samples, ds.T, ds.V
        self.xy = torch.from_numpy(np.ascontiguousarray(ds.segs_data_np[:, :2])).to(device).reshape(self.N, 2, self.T * self.V).contiguous()
        self.mats = torch.from_numpy(np.ascontiguousarray(ds.trans_mats)).to(device)
        self.meta = torch.from_numpy(ds.segs_meta.astype(np.int64))
        self.frames = torch.from_numpy(ds.segs_ids.astype(np.int32))

    def gather(self, index: torch.Tensor) -> torch.Tensor:
        from .. import ops
        return ops.gather_transform(self.xy, self.mats, index.to(self.xy.device, non_blocking=True), self.T, self.V)


# ---- the frame-resident form (`dataset_resident: 'frames'`) --------------------------------------------------------------
def check_window_rows(win_row: np.ndarray, traj_ptr: np.ndarray, T: int, step: int) -> None:
    """Window s covers the rows win_row[s] + t * step, t < T, of a frame table in which trajectory k is the rows
    traj_ptr[k] .. traj_ptr[k + 1].  ValueError unless the table has fewer than 2^31 rows (win_row is int32 on the device) and
    every window stays inside the trajectory its first row lies in."""
    traj_ptr = np.asarray(traj_ptr, dtype=np.int64)
    F = int(traj_ptr[-1])
    if F >= 2 ** 31:
        raise ValueError(f"the frame table has {F} rows; the device table addresses fewer than 2^31")
    w = np.asarray(win_row, dtype=np.int64)
    if w.size == 0:
        raise ValueError("no trajectory is long enough for one window")
    k = np.searchsorted(traj_ptr, w, side='right') - 1
    ok = (w >= 0) & (w < F)
    end = traj_ptr[np.clip(k + 1, 0, len(traj_ptr) - 1)]
    bad = np.flatnonzero(~ok | (w + (T - 1) * step >= end))
    if bad.size:
        s = int(bad[0])
        raise ValueError(f"window {s} (rows {int(w[s])} + t * {step}, t < {T}) leaves its trajectory; {bad.size} such windows")


class _WindowFrameIds:
    """`segs_ids` [N, T] without the array: entry [s, t] is frame_id[win_row[s] + t * step].  Indexing with an integer, a slice,
    a mask or an index array (and an optional second index along T) gives what the int64 array would give."""

    def __init__(self, frame_id: np.ndarray, win_row: np.ndarray, T: int, step: int) -> None:
        self._id, self._row, self._off = frame_id, win_row, step * np.arange(T, dtype=np.int64)
        self.shape, self.dtype, self.ndim = (len(win_row), T), np.dtype(np.int64), 2

    def __len__(self) -> int:
        return self.shape[0]

    def __getitem__(self, key):
        key, cols = (key[0], key[1]) if isinstance(key, tuple) else (key, slice(None))
        rows = np.asarray(self._row[key], dtype=np.int64)
        return self._id[rows[..., None] + self._off].astype(np.int64)[..., cols]

    def __array__(self, dtype=None, copy=None):
        a = self[:]
        return a if dtype is None else a.astype(dtype)


class PoseFramesRobust:
    """PoseDatasetRobust with ONE normalised row per trajectory frame instead of one array per window: overlapping windows share
    their frames, so host and device hold 1 / T (at seg_stride 1) of the window table, and `seg_len` / `seg_stride` only change
    the small index `win_row`.  Same constructor arguments, same items in the same order, bit for bit.

    frame_xy [F, 2, V] f32: the kept trajectories, concatenated in trajectory order, normalised exactly as the window path
    normalises (scaler on the 34 columns with zeros as missing -> (x, y, 1) -> kp18 -> headless; float64, then float32);
    frame_id [F] int32; win_row [N] int32: the row of each window's first frame, windows in `build_windows` order, window s =
    rows win_row[s] + t * seg_stride, t < T; segs_meta [N, 4]; segs_ids: [N, T] formed on indexing.

    This class never allocates an [N, T, .] float array: every float table here has one row per frame, and `window(s)` /
    `__getitem__` form one window on demand."""

    def __init__(self, path_to_robust_data: str, split: str = 'train', exp_dir: str = '', num_transform: int = 5,
                 seg_len: int = 12, seg_stride: int = 1, vid_res: Sequence[int] = (1080, 720), num_coords: int = 2,
                 normalize_pose: bool = True, kp18_format: bool = False, headless: bool = False, debug: bool = False,
                 scaler=None) -> None:
        self.split, self.num_coords, self.seg_len, self.step = split, num_coords, seg_len, int(seg_stride)
        self.num_transform = max(1, int(num_transform))
        self.trans_mats = AE_TRANS_MATS[:self.num_transform] if num_transform > 0 else AE_TRANS_MATS[:1]
        trajs, self.scaler = robust_front_end(path_to_robust_data, split, exp_dir, seg_len, seg_stride, vid_res,
                                              normalize_pose, debug, scaler)
        span = (seg_len - 1) * self.step                       # first to last row of a window
        lengths = np.array([len(f) for f, _ in trajs.values()], dtype=np.int64)
        self.traj_ptr = np.concatenate([[0], np.cumsum(lengths)])
        rows, metas = [], []
        for (tid, (frames, _)), off, n in zip(trajs.items(), self.traj_ptr, lengths):
            starts = np.arange(0, n - span)
            scene, clip = (int(v) for v in tid.split('_')[0].split('-'))
            person = int(tid.split('_')[1])
            rows.append(off + starts)
            metas.append(np.stack([np.full(starts.size, scene), np.full(starts.size, clip), np.full(starts.size, person),
                                   frames[starts]], 1).astype(np.int64))
        win_row = np.concatenate(rows)
        check_window_rows(win_row, self.traj_ptr, seg_len, self.step)
        self.win_row = win_row.astype(np.int32)
        self.frame_id = np.concatenate([f for f, _ in trajs.values()]).astype(np.int32)
        X = np.vstack([c for _, c in trajs.values()])
        if normalize_pose:
            X, _ = scale_robust(X, self.scaler)
        data = pose_layout(X, kp18_format, headless)                                       # [F, V, 3] float64
        self.frame_xy = np.ascontiguousarray(np.transpose(data[..., :2], (0, 2, 1)).astype(np.float32))
        self.segs_meta = np.concatenate(metas, 0)
        self.metadata = self.segs_meta
        self.segs_ids = _WindowFrameIds(self.frame_id, self.win_row, seg_len, self.step)
        self.num_samples, self.C, self.T, self.V = len(self.win_row), 3, seg_len, self.frame_xy.shape[2]

    def __len__(self) -> int:
        return self.num_transform * self.num_samples

    def window(self, s: int) -> np.ndarray:
        """Window s as the window class stores it: [3, T, V] f32 = (x, y, 1)."""
        xy = self.frame_xy[int(self.win_row[s]) + self.step * np.arange(self.T)]           # [T, 2, V]
        return np.concatenate([np.transpose(xy, (1, 0, 2)), np.ones((1, self.T, self.V), np.float32)], 0)

    def __getitem__(self, index: int):
        s, t = index % self.num_samples, index // self.num_samples
        data = apply_pose_transform(self.window(s), self.trans_mats[t])[:self.num_coords]
        return [data, t, self.segs_meta[s], self.segs_ids[s]]

    def to_device(self, device="cuda") -> "FrameWindows":
        return FrameWindows(self, device)


class _WindowFramesTorch:
    """`DeviceWindows.frames` for the frame table: `frames[s]` -> int32 [len(s), T] frame ids of the windows `s` (host)."""

    def __init__(self, frame_id: torch.Tensor, win_row: torch.Tensor, T: int, step: int) -> None:
        self._id, self._row, self._off = frame_id, win_row.long(), step * torch.arange(T)

    def __getitem__(self, s) -> torch.Tensor:
        return self._id[self._row[s][..., None] + self._off]


class FrameWindows:
    """The frame table resident in HBM: fxy [F, 2, V] f32, win_row [N] int32 and the transform matrices on the device; meta,
    frame_id and win_row also on the host.  `gather(index)` = one HIP kernel (`coskad_gather_frames_f32`) that forms the batch
    [B, 2, T, V] from the windows' frames: the same bits as `DeviceWindows.gather`, which `DeviceLoader` may be given instead."""

    def __init__(self, ds: PoseFramesRobust, device="cuda") -> None:
        if ds.num_coords != 2:
            raise ValueError("the device loader serves the (x, y) layout (num_coords = 2)")
        self.ds = ds
        self.N, self.T, self.V, self.step = ds.num_samples, ds.T, ds.V, ds.step
        self.fxy = torch.from_numpy(ds.frame_xy).to(device)
        self.mats = torch.from_numpy(np.ascontiguousarray(ds.trans_mats)).to(device)
        self.meta = torch.from_numpy(ds.segs_meta.astype(np.int64))
        self.frame_id, self.win_row = torch.from_numpy(ds.frame_id), torch.from_numpy(ds.win_row)
        self.win_row_dev = self.win_row.to(device)
        self.frames = _WindowFramesTorch(self.frame_id, self.win_row, self.T, self.step)

    def gather(self, index: torch.Tensor) -> torch.Tensor:
        from .. import ops
        return ops.gather_frames(self.fxy, self.win_row_dev, self.mats, index.to(self.fxy.device, non_blocking=True), self.T,
                                 self.V, self.step)


class DeviceLoader:
    """Batches `[x (device), trans_idx, meta, frames]` like the reference's DataLoader over PoseDatasetRobust; rank r of
    W takes items r, r+W, ... of the (optionally shuffled) index list with the tail wrap-padded to ceil(n / W) items per
    rank, as DistributedSampler does under Lightning DDP: every rank runs the same number of batches (and collectives)."""

    def __init__(self, windows: "DeviceWindows | FrameWindows", batch_size: int, shuffle: bool = False, seed: int = 0, rank: int = 0,
                 world: int = 1) -> None:
        self.w, self.batch_size, self.shuffle, self.seed, self.rank, self.world = windows, batch_size, shuffle, seed, rank, world
        self.epoch = 0

    def __len__(self) -> int:
        n = (len(self.w.ds) + self.world - 1) // self.world
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self) -> Iterator[List[torch.Tensor]]:
        n = len(self.w.ds)
        if self.shuffle:
            idx = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + self.epoch))
            self.epoch += 1
        else:
            idx = torch.arange(n)
        from ..parallel import shard_indices
        idx = idx[shard_indices(n, self.rank, self.world)]
        for i in range(0, idx.numel(), self.batch_size):
            j = idx[i:i + self.batch_size]
            s = j % self.w.N
            yield [self.w.gather(j), j // self.w.N, self.w.meta[s], self.w.frames[s]]


def get_dataset_and_loader(args, split: str = 'train', validation: bool = False, rank: int = 0, world: int = 1,
                           device="cuda"):
    """utils/dataset.py:284-327 for `normalization_strategy == 'robust'`; `args` carries the reference's dataset_* keys
    (with or without the prefix).  Returns (dataset, loader[, val_dataset, val_loader])."""
    def g(name, default=None):
        return getattr(args, 'dataset_' + name, getattr(args, name, default))
    common = dict(exp_dir=g('exp_dir', getattr(args, 'ckpt_dir', '')), num_transform=g('num_transform', 5),
                  seg_len=g('seg_len', 12), vid_res=g('vid_res', [1080, 720]), num_coords=getattr(args, 'num_coords', 2),
                  normalize_pose=g('normalize_pose', True), kp18_format=g('kp18_format', False),
                  headless=g('headless', False), debug=getattr(args, 'debug', False))
    root = g('path_to_robust', getattr(args, 'data_dir', ''))
    bs = g('batch_size', 2048)
    # `dataset_resident` (not a key of the reference's yamls): 'windows' keeps one array per window in HBM, 'frames' one row per
    # trajectory frame and forms the windows in the gather kernel; the batches are the same bits
    resident = g('resident', 'windows')
    if resident not in ('windows', 'frames'):
        raise ValueError(f"dataset_resident: expected 'windows' or 'frames', got {resident!r}")
    cls = PoseFramesRobust if resident == 'frames' else PoseDatasetRobust
    ds = cls(root, split=split, seg_stride=g('seg_stride', 1) if split == 'train' else 1, **common)
    loader = DeviceLoader(ds.to_device(device), bs, shuffle=(split == 'train'), seed=getattr(args, 'seed', 0), rank=rank, world=world)
    if not validation:
        return ds, loader
    vds = cls(root, split='validation', seg_stride=1, scaler=ds.scaler, **common)
    return ds, loader, vds, DeviceLoader(vds.to_device(device), bs, rank=rank, world=world)
