"""Frame-level scoring of a validation pass on the device (csrc/score_frames.hip).

`eval_utils.score_dataset` re-derives, at every call, everything that depends only on the window table (`trans`, `meta`, `frames`) of
the validation set: which windows cover which frame of which person, which persons belong to which clip, where a clip's frames land in
the concatenated score vector.  A `ScorePlan` derives that ONCE, as index tables on the device; `score_dataset_device` then runs a
handful of small deterministic kernels per call and brings one scalar to the host.  The semantics are `score_dataset`'s (and so those of
oracle/ref_scoring.py): exact zeros count as missing, optional absence padding per person, max over persons, human-related masks before
smoothing, shift by 11 + gaussian_filter1d(sigma 30, `reflect`), mean over transformations, tie-aware AUC.

`score_report_device` goes on from the same frame scores to the rest of what the reference's evaluation prints (eval_COSKAD.py:222-242):
the AUC of every clip and of the whole test set per transformation and the ROC thresholds, as a `ScoreReport` (csrc/score_report.hip);
`eval_utils.score_report` forms the same report on the host with sklearn and is its yardstick.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

SIGMA = 30
RADIUS = int(4.0 * SIGMA + 0.5)      # gaussian_filter1d's truncate = 4.0
TILE = 256                           # outputs per workgroup of the smoothing kernel (coskad_score_tile())
PAD_ROW_MAX = 8192                   # frames of one person's row in the padding kernel's LDS (coskad_score_pad_row_max())
_I32_MAX = 2 ** 31 - 1


def gaussian_taps(sigma: float = SIGMA, radius: int = RADIUS) -> np.ndarray:
    """taps[k], k = 0 .. radius: the weight of gaussian_filter1d(sigma) at offset +-k -- exp(-0.5 / sigma^2 * x^2) over
    x = -radius .. radius, normalised by its sum (the operations in scipy's order, so the values are scipy's to the bit)."""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def segment_tiles(segments) -> np.ndarray:
    """[n_tiles, 3] int64 rows (segment start, segment end, tile start): the smoothing kernel's work list for segments [start, end) of
    the concatenated vector, TILE outputs per tile; an empty segment has no tile."""
    rows = [(int(a), int(b), s) for a, b in np.asarray(segments).reshape(-1, 2).tolist() for s in range(int(a), int(b), TILE)]
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


class ScorePlan:
    """Index tables of one validation set's scoring, built once from its window table.

    persons      person_keys [P, 4] = the unique (t, scene, clip, person) with t < num_transform and (scene, clip) in `gts`, sorted;
                 person_clip [P] the clip's slot in sorted(gts), person_n [P] its length; row_ptr [P + 1]: person p's frames are the
                 entries row_ptr[p] .. row_ptr[p + 1] of the person x frame vector
    window CSR   win_ptr [row_ptr[P] + 1], win_idx: the windows (positions in the score vector) whose frame list holds that frame of
                 that person, in ascending order
    person CSR   pc_ptr [num_transform * C + 1]: the persons of (t, clip slot c) are pc_ptr[t C + c] .. pc_ptr[t C + c + 1]
    output       clips in sorted(gts) order, `hr_masks` applied: out_clip / out_frame [F] the source of every output position,
                 segments [C, 2] each clip's [start, end), tiles [n_tiles, 3] = (start, end, tile start), gt the concatenated ground truth
    taps         gaussian_taps() as float64
    Device tensors are int32 / float64 (`win_ptr` ... `tiles`, `gt_dev`, `taps`); the numpy attributes above stay on the host.
    """

    def __init__(self, trans, meta, frames, gts: Dict[Tuple[int, int], np.ndarray], num_transform: int, pad_size: int = -1,
                 hr_masks: Optional[Dict[Tuple[int, int], np.ndarray]] = None, device=None) -> None:
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.num_transform, self.pad_size = int(num_transform), int(pad_size)
        if self.num_transform < 1:
            raise ValueError(f"num_transform = {num_transform}")
        # the tables as they came, for matches(): exact comparison, never an assumption
        self._tables = tuple(torch.as_tensor(t).detach().clone() for t in (trans, meta, frames))
        tr, me, fr = _host(trans).astype(np.int64).reshape(-1), _host(meta).astype(np.int64), _host(frames).astype(np.int64)
        if fr.ndim != 2 or me.ndim != 2 or me.shape[1] < 3 or not (tr.shape[0] == me.shape[0] == fr.shape[0]):
            raise ValueError(f"window table: trans {tr.shape}, meta {me.shape}, frames {fr.shape}")
        self.N, self.T = int(fr.shape[0]), int(fr.shape[1])
        keys = sorted(gts.keys())
        if not keys:
            raise ValueError("no ground truth clips")
        self.clip_keys = keys
        C = self.n_clips = len(keys)
        lengths = np.array([int(np.asarray(gts[k]).shape[0]) for k in keys], dtype=np.int64)

        # clip slot of every window (-1: a clip without ground truth), through one integer code per (scene, clip)
        karr = np.array(keys, dtype=np.int64).reshape(-1, 2)
        sc0 = min(int(karr[:, 0].min()), int(me[:, 0].min())) if self.N else int(karr[:, 0].min())
        cl0 = min(int(karr[:, 1].min()), int(me[:, 1].min())) if self.N else int(karr[:, 1].min())
        span = (max(int(karr[:, 1].max()), int(me[:, 1].max()) if self.N else cl0) - cl0) + 1
        kcode = (karr[:, 0] - sc0) * span + (karr[:, 1] - cl0)           # ascending, as the keys are sorted
        wcode = (me[:, 0] - sc0) * span + (me[:, 1] - cl0)
        pos = np.minimum(np.searchsorted(kcode, wcode), C - 1)
        slot = np.where(kcode[pos] == wcode, pos, -1)
        keep = (tr >= 0) & (tr < self.num_transform) & (slot >= 0)
        widx = np.nonzero(keep)[0]

        # persons: unique (t, slot, person) in sorted order, so the persons of one (t, clip) are contiguous
        pe = me[widx, 2]
        pe0 = int(pe.min()) if widx.size else 0
        pspan = (int(pe.max()) - pe0 + 1) if widx.size else 1
        pcode = (tr[widx] * C + slot[widx]) * pspan + (pe - pe0)
        ucode, pid = np.unique(pcode, return_inverse=True)
        P = self.n_persons = int(ucode.shape[0])
        tc = ucode // pspan
        self.person_clip = (tc % C).astype(np.int64)
        self.person_n = lengths[self.person_clip] if P else np.zeros(0, dtype=np.int64)
        self.person_keys = np.stack([tc // C, karr[self.person_clip, 0], karr[self.person_clip, 1], ucode % pspan + pe0], 1) \
            if P else np.zeros((0, 4), dtype=np.int64)
        row_ptr = np.concatenate([[0], np.cumsum(self.person_n)]).astype(np.int64)
        pc_ptr = np.searchsorted(tc, np.arange(self.num_transform * C + 1))
        self.n_max = int(self.person_n.max()) if P else 0
        if self.pad_size != -1 and self.n_max > PAD_ROW_MAX:
            raise ValueError(f"absence padding on the device holds a person's row in LDS: clips of up to {PAD_ROW_MAX} frames, got "
                             f"{self.n_max} (`device_scoring: false` scores such a set on the host route)")

        # window CSR: (person, frame) -> covering windows, ascending
        f0 = fr[widx] - 1                                                # `frames - 1`: eval_utils.py:72
        bad = (f0 < 0) | (f0 >= self.person_n[pid][:, None]) if widx.size else np.zeros((0, self.T), dtype=bool)
        if bad.any():
            w = int(widx[np.nonzero(bad.any(1))[0][0]])
            raise ValueError(f"window {w}: frame numbers {fr[w].tolist()} outside 1..{int(lengths[slot[w]])} of clip "
                             f"{keys[int(slot[w])]}")
        entry = (row_ptr[pid][:, None] + f0).reshape(-1)
        PF = int(row_ptr[-1])
        if PF > _I32_MAX or entry.shape[0] > _I32_MAX:
            raise ValueError(f"scoring tables beyond int32: {PF} person frames, {entry.shape[0]} window frames")
        order = np.argsort(entry, kind="stable")
        win_idx = np.repeat(widx, self.T)[order]
        win_ptr = np.concatenate([[0], np.cumsum(np.bincount(entry, minlength=PF))])

        # output layout: clips in sorted order, human-related masks applied to the clip score and the ground truth
        hr_masks = hr_masks or {}
        oc, of, gt_parts, segs, start = [], [], [], [], 0
        for c, k in enumerate(keys):
            src = np.arange(int(lengths[c]))
            g = np.asarray(gts[k])
            if k in hr_masks:
                src, g = src[hr_masks[k]], g[hr_masks[k]]
            oc.append(np.full(src.shape[0], c, dtype=np.int64)); of.append(src); gt_parts.append(g)
            end = start + int(src.shape[0])
            segs.append((start, end))
            start = end
        self.F = start
        if self.F > _I32_MAX:
            raise ValueError(f"{self.F} output frames: beyond int32")
        self.segments = np.array(segs, dtype=np.int64).reshape(-1, 2)
        self._src_frames = np.concatenate(of)
        self.gt = np.concatenate(gt_parts)
        tiles = segment_tiles(self.segments)
        self.n_tiles = int(tiles.shape[0])

        def dev(a, dtype=torch.int32):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.device)
        self.win_ptr, self.win_idx, self.row_ptr, self.pc_ptr = dev(win_ptr), dev(win_idx), dev(row_ptr), dev(pc_ptr)
        self.out_clip, self.out_frame = dev(np.concatenate(oc)), dev(np.concatenate(of))
        self.tiles = dev(tiles)
        self.gt_dev = dev(self.gt != 0)
        self.taps = dev(gaussian_taps(), torch.float64)
        self.segments_dev = dev(self.segments)
        self._report_tables = None

    def report_tables(self):
        """The report kernels' tables of this plan's segments (`report_tables`), built at the first report and kept."""
        if self._report_tables is None:
            self._report_tables = report_tables(self.segments, self.F, self.device)
        return self._report_tables

    def matches(self, trans, meta, frames) -> bool:
        """True only if the tables are the ones this plan was built from: same shapes, every entry equal (compared where the plan's
        copies live; a copy is as large as the table, 8 + 32 + 4 T bytes per window for int64 trans / meta and int32 frames)."""
        for mine, other in zip(self._tables, (trans, meta, frames)):
            other = torch.as_tensor(other)
            if mine.shape != other.shape:
                return False
            other = other.to(mine.device)
            if not (torch.equal(mine, other) if other.dtype == mine.dtype else torch.equal(mine.long(), other.long())):
                return False
        return True

    def same_setting(self, gts, num_transform: int, pad_size: int, hr_masks) -> bool:
        """True if ground truth, masks and parameters are the ones this plan was built with (what `matches` does for the tables)."""
        if int(num_transform) != self.num_transform or int(pad_size) != self.pad_size or sorted(gts.keys()) != self.clip_keys:
            return False
        hr_masks = hr_masks or {}
        parts = [np.asarray(gts[k])[hr_masks[k]] if k in hr_masks else np.asarray(gts[k]) for k in self.clip_keys]
        segs = np.cumsum([0] + [p.shape[0] for p in parts])
        if not np.array_equal(np.stack([segs[:-1], segs[1:]], 1), self.segments) or not np.array_equal(np.concatenate(parts), self.gt):
            return False
        src = np.concatenate([np.arange(len(gts[k]))[hr_masks[k]] if k in hr_masks else np.arange(len(gts[k])) for k in self.clip_keys])
        return np.array_equal(src, self._src_frames)


def frame_scores_device(window_scores, plan: ScorePlan):
    """The kernels of `score_dataset_device` up to the smoothed frame scores: -> (per_t [num_transform, F], their mean [F]), float64 on
    the device."""
    from .. import _lib, ops
    s = torch.as_tensor(window_scores).reshape(-1)
    if not s.is_cuda:
        raise _lib.CoskadHipError(f"score_dataset_device: expected window scores on the GPU, got device {s.device}; frame scoring on "
                                  "the device runs only on the HIP extension (no CPU fallback; `score_dataset` is the host route)")
    if s.device != plan.win_ptr.device:
        raise ValueError(f"score_dataset_device: scores on {s.device}, plan on {plan.win_ptr.device}")
    if s.numel() != plan.N:
        raise ValueError(f"score_dataset_device: {s.numel()} window scores for a plan of {plan.N} windows")
    if plan.F == 0:
        raise ValueError("score_dataset_device: no frames to score")
    if s.dtype not in (torch.float32, torch.float64):
        s = s.double()
    s = s.contiguous()
    nt, F = plan.num_transform, plan.F
    if plan.n_persons:
        pf = ops.score_person_frames(s, plan.win_ptr, plan.win_idx)
        if plan.pad_size != -1:
            ops.score_pad_(pf, plan.row_ptr, plan.pad_size, plan.n_max)
        raw = ops.score_clip_max(pf, plan.row_ptr, plan.pc_ptr, plan.out_clip, plan.out_frame, plan.n_clips, nt)
    else:
        raw = torch.zeros(nt, F, dtype=torch.float64, device=s.device)       # no detections at all: every clip scores 0
    return ops.score_smooth(raw, plan.tiles, plan.taps)


def score_dataset_device(window_scores, plan: ScorePlan):
    """`score_dataset` on the device, from a ready plan: -> (AUC: float, per_t: Tensor [num_transform, F] float64 on the device,
    concatenated gt: np.ndarray).  Window scores are a float32 or float64 tensor on the GPU, one per row of the plan's window table."""
    per_t, mean = frame_scores_device(window_scores, plan)
    return auc_device(mean, plan.gt_dev), per_t, plan.gt


def auc_device(scores: torch.Tensor, gt: torch.Tensor) -> float:
    """roc_auc_score(gt, scores) for float64 scores and an int32 ground truth (non-zero = positive) on the GPU.  Ordering is plumbing
    (torch.sort / cumsum); the tie-aware Mann-Whitney statistic itself is formed by the kernel, in int64.  One device -> host copy."""
    from .. import ops
    order_scores, perm = torch.sort(scores)
    gt_sorted = gt[perm]
    auc, n_pos, n_neg = ops.score_auc(order_scores, gt_sorted, torch.cumsum(gt_sorted == 0, 0)).tolist()
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return float(auc)


# ---- the evaluation report: per-clip AUCs, per-transformation AUCs and ROC thresholds (csrc/score_report.hip) ----

REPORT_TILE = 256                    # elements per workgroup of the report kernels (coskad_score_report_tile())


def _nanmean(a) -> float:
    a = np.asarray(a, dtype=np.float64)
    a = a[~np.isnan(a)]
    return float(a.mean()) if a.size else float("nan")


class ScoreReport:
    """What the reference's evaluation prints beside the final AUC (eval_COSKAD.py:222-253), as plain Python / numpy on the host.

    auc              the final AUC: roc_auc_score(gt, mean over the transformations)
    auc_t [nt]       the AUC of the concatenated test set per transformation
    thresholds_t     per transformation the array tr[idx] of the reference's ROC(): where the ROC curve crosses tpr = 1 - fpr
    clip_auc [nt, C] the AUC of every clip per transformation; NaN where the clip's ground truth has one class or no frame
    clip_auc_final   [C]: the same on the mean over the transformations
    clip_auc_mean_t  [nt]: the mean over the defined clips (the last `average_score` the reference prints for a transformation)
    clip_keys        [(scene, clip)] in the order of the columns; n_pos / n_neg [C] int64: the clips' positive / negative frames
    segments [C, 2]  each clip's [start, end) in frame_scores [F], the final per-frame scores
    """

    def __init__(self, auc, auc_t, thresholds_t, clip_auc, clip_auc_final, clip_keys, n_pos, n_neg, segments, frame_scores) -> None:
        self.auc = float(auc)
        self.auc_t = np.asarray(auc_t, dtype=np.float64).reshape(-1)
        self.thresholds_t = [np.asarray(t, dtype=np.float64).reshape(-1) for t in thresholds_t]
        self.clip_keys = [tuple(int(v) for v in k) for k in clip_keys]
        C = len(self.clip_keys)
        self.clip_auc = np.asarray(clip_auc, dtype=np.float64).reshape(self.auc_t.shape[0], C)
        self.clip_auc_final = np.asarray(clip_auc_final, dtype=np.float64).reshape(C)
        self.clip_auc_mean_t = np.array([_nanmean(row) for row in self.clip_auc], dtype=np.float64)
        self.n_pos, self.n_neg = np.asarray(n_pos, dtype=np.int64).reshape(C), np.asarray(n_neg, dtype=np.int64).reshape(C)
        self.segments = np.asarray(segments, dtype=np.int64).reshape(C, 2)
        self.frame_scores = np.asarray(frame_scores, dtype=np.float64).reshape(-1)

    def lines(self):
        """The reference's log lines, in its order and wording; a clip whose AUC is undefined prints `nan` (the reference prints the
        previous clip's value there)."""
        nt, C = self.clip_auc.shape
        for t in range(nt):
            for k, key in enumerate(self.clip_keys):
                yield 'transf: {}/{}, clip: {},{}/{}, score: {} average_score: {}'.format(
                    t + 1, nt, key, k + 1, C, self.clip_auc[t, k], _nanmean(self.clip_auc[t, :k + 1]))
            yield 'Test set score for transformation {}'.format(t + 1)
            yield '{}'.format(self.thresholds_t[t])
            yield 'auc = {}'.format(self.auc_t[t])
        yield 'final AUC score: {}'.format(self.auc)

    def to_dict(self) -> dict:
        def clean(v):
            if isinstance(v, (list, tuple, np.ndarray)):
                return [clean(x) for x in v]
            if isinstance(v, (float, np.floating)):
                return None if np.isnan(v) else (str(float(v)) if np.isinf(v) else float(v))
            return int(v)
        return {name: clean(getattr(self, name)) for name in ("auc", "auc_t", "thresholds_t", "clip_auc", "clip_auc_final",
                                                              "clip_auc_mean_t", "clip_keys", "n_pos", "n_neg", "segments")}

    def save(self, directory: str) -> None:
        """`report.json` (NaN as null, an infinite threshold as the string "inf") and `<scene>_<clip>.npy`, each clip's final scores."""
        import json
        import os
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "report.json"), "w") as f:
            json.dump(self.to_dict(), f, indent=1, allow_nan=False)
        for (sc, cl), (a, b) in zip(self.clip_keys, self.segments.tolist()):
            np.save(os.path.join(directory, f"{sc}_{cl}.npy"), self.frame_scores[a:b])


def check_segments(segments, F: int) -> np.ndarray:
    """[C, 2] int64 if the segments are [start, end) ranges inside [0, F], ascending and not overlapping; ValueError otherwise."""
    seg = np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    flat = seg.reshape(-1)
    if seg.shape[0] == 0 or flat[0] < 0 or flat[-1] > F or np.any(np.diff(flat) < 0):
        raise ValueError(f"segments: expected [start, end) ranges inside [0, {F}], ascending and not overlapping, got {seg.tolist()[:8]}")
    return seg


def report_tables(segments, F: int, device=None):
    """The index tables of the report kernels for segments [C, 2] of F frames, on `device` (default: where the segments are):
    (segment key [F] int32 -- 2 c + 1 inside segment c, even between segments --, tile_ptr [C + 1] int32, the whole vector's segment
    [1, 2] and its tile_ptr [2]).  torch index arithmetic where the segments live: nothing comes to the host."""
    seg = torch.as_tensor(segments).reshape(-1, 2).to(torch.int64)
    device = seg.device if device is None else torch.device(device)
    key = torch.bucketize(torch.arange(F, device=seg.device), seg.reshape(-1), right=True).to(torch.int32)
    tiles = torch.div(seg[:, 1] - seg[:, 0] + (REPORT_TILE - 1), REPORT_TILE, rounding_mode="floor").clamp_min(0)
    tile_ptr = torch.cat([tiles.new_zeros(1), torch.cumsum(tiles, 0)]).to(torch.int32)
    whole = torch.tensor([[0, F]], dtype=torch.int32)
    whole_ptr = torch.tensor([0, (F + REPORT_TILE - 1) // REPORT_TILE], dtype=torch.int32)
    return tuple(t.to(device).contiguous() for t in (key, tile_ptr, whole, whole_ptr))


def report_from_frame_scores(per_t: torch.Tensor, mean: torch.Tensor, gt_dev: torch.Tensor, segments_dev: torch.Tensor, clip_keys,
                             tables=None, segments=None) -> ScoreReport:
    """The report from smoothed frame scores on the GPU: per_t [nt, F] and mean [F] float64, gt_dev [F] int32 (non-zero = positive),
    segments_dev [C, 2] int32 (ascending, not overlapping; `segments`, the same on the host, is checked when given), `tables` =
    report_tables(...) of those segments when the caller keeps them.

    Ordering is plumbing, as in `auc_device`: one stable sort of the nt + 1 rows by score gives the whole vector's order, one stable
    sort of that by segment key gives every clip's order in place.  Then four launches form all (nt + 1) x (C + 1) AUCs -- clips, then
    the whole vector -- and two the thresholds of the nt rows, whatever C is; everything lands in one buffer that comes to the host in
    one copy.  The whole-vector AUC of the mean row is `auc_device(mean, gt_dev)` to the bit."""
    from .. import _lib, ops
    if not (per_t.is_cuda and mean.is_cuda):
        raise _lib.CoskadHipError(f"report_from_frame_scores: expected frame scores on the GPU, got {per_t.device} / {mean.device}; the "
                                  "report kernels run only on the HIP extension (no CPU fallback; `score_report` is the host route)")
    if per_t.dim() != 2 or per_t.shape[0] < 1 or per_t.shape[1] < 1 or mean.shape != per_t.shape[1:]:
        raise ValueError(f"report_from_frame_scores: per_t {tuple(per_t.shape)}, mean {tuple(mean.shape)}")
    nt, F = per_t.shape
    C = len(clip_keys)
    if C < 1 or tuple(segments_dev.shape) != (C, 2) or gt_dev.shape != (F,):
        raise ValueError(f"report_from_frame_scores: {C} clips, segments {tuple(segments_dev.shape)}, gt {tuple(gt_dev.shape)} for "
                         f"{F} frames")
    if segments is not None:
        check_segments(segments, F)
    key, tile_ptr, whole, whole_ptr = tables if tables is not None else report_tables(segments_dev, F)
    R = nt + 1
    rows = torch.cat([per_t.double(), mean.double()[None]], 0)
    s_all, perm = torch.sort(rows, dim=1, stable=True)                   # every row ascending: the whole vector's order
    gt_all = gt_dev.to(torch.int32)[perm]
    _, by_seg = torch.sort(key[perm], dim=1, stable=True)                # ... then by segment: each clip ascending, in its own range
    s_seg, gt_seg = torch.gather(s_all, 1, by_seg), torch.gather(gt_all, 1, by_seg)
    n_clip, n_whole, n_thr = R * C * 3, R * 3, nt * 3
    buf = torch.empty(n_clip + n_whole + n_thr + 2 * C + F, device=rows.device, dtype=torch.float64)
    ops.score_report_auc(s_seg, gt_seg, torch.cumsum(gt_seg == 0, 1), segments_dev, tile_ptr, F // REPORT_TILE + C,
                         out=buf[:n_clip].view(R, C, 3))
    cum_all = torch.cumsum(gt_all == 0, 1)
    ops.score_report_auc(s_all, gt_all, cum_all, whole, whole_ptr, (F + REPORT_TILE - 1) // REPORT_TILE,
                         out=buf[n_clip:n_clip + n_whole].view(R, 1, 3))
    ops.score_report_thresholds(s_all[:nt], cum_all[:nt], out=buf[n_clip + n_whole:n_clip + n_whole + n_thr].view(nt, 3))
    buf[n_clip + n_whole + n_thr:n_clip + n_whole + n_thr + 2 * C].copy_(segments_dev.reshape(-1))
    buf[n_clip + n_whole + n_thr + 2 * C:].copy_(rows[nt])
    host = buf.cpu().numpy()                                             # the one device -> host copy
    clip = host[:n_clip].reshape(R, C, 3)
    whole_h = host[n_clip:n_clip + n_whole].reshape(R, 3)
    thr = host[n_clip + n_whole:n_clip + n_whole + n_thr].reshape(nt, 3)
    seg_h = host[n_clip + n_whole + n_thr:n_clip + n_whole + n_thr + 2 * C].reshape(C, 2).astype(np.int64)
    if np.any(clip[R - 1, :, 1] < 0):
        bad = int(np.nonzero(clip[R - 1, :, 1] < 0)[0][0])
        raise ValueError(f"report_from_frame_scores: segment {bad} = {seg_h[bad].tolist()} does not lie in [0, {F}]")
    if whole_h[R - 1, 1] == 0 or whole_h[R - 1, 2] == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return ScoreReport(auc=float(whole_h[R - 1, 0]), auc_t=whole_h[:nt, 0], thresholds_t=[thr[t, 1:1 + int(thr[t, 0])] for t in range(nt)],
                       clip_auc=clip[:nt, :, 0], clip_auc_final=clip[R - 1, :, 0], clip_keys=clip_keys, n_pos=clip[R - 1, :, 1],
                       n_neg=clip[R - 1, :, 2], segments=seg_h, frame_scores=host[n_clip + n_whole + n_thr + 2 * C:])


def score_report_device(window_scores, plan: ScorePlan):
    """`score_dataset_device`'s pipeline, then the report: -> (ScoreReport, per_t [num_transform, F] float64 on the device,
    concatenated gt: np.ndarray); `report.auc` is what `score_dataset_device` returns for the same scores and plan."""
    per_t, mean = frame_scores_device(window_scores, plan)
    report = report_from_frame_scores(per_t, mean, plan.gt_dev, plan.segments_dev, plan.clip_keys, tables=plan.report_tables(),
                                      segments=plan.segments)
    return report, per_t, plan.gt
