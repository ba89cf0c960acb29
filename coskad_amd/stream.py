"""Online scoring: live pose tracks in, frame by frame; window scores and per-person frame scores out.

The offline route needs a finished Morais CSV tree (`PoseDatasetRobust` / `PoseFramesRobust`) and a `ScorePlan` of the complete window
table.  Here the same arithmetic runs one frame at a time: `StreamScorer.push` takes the skeletons a tracker found in one frame,
normalises them on the device as `bbox_centre_coordinates` / `scale_robust` / `pose_layout` do, keeps the last R = (T - 1) seg_stride + 1
rows of every track in a ring, scores the window of every track that has one with the wrapper's ordinary eval scoring, and hands out
  * the window scores at once, and
  * the frame score of a (track, frame) R - 1 rows later, when no further window can cover it,
by the rules of `eval_utils.person_frame_scores` -- so replaying a test split reproduces what eval_COSKAD.py computes, bit for bit.
Kernels: csrc/stream.hip.  `StreamPlan` is the host's bookkeeping (slots, row counts, frame ids, readiness) and needs no native library.
"""
from __future__ import annotations

import heapq
from collections import deque
from typing import Dict, Hashable, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

N_RAW = 34                      # a raw row: x1, y1, ..., x17, y17
_STAGES = 8                     # pinned staging buffers in rotation: a push never waits for the upload of the one before


class PushPlan(NamedTuple):
    """One push as the launches need it: per detection its slot, whether it starts its track and the position of its window in the
    output (-1: no window yet); per ready track its id, slot and the frame id of its window's first row (the row that becomes final)."""
    slots: List[int]
    reset: List[int]
    out_index: List[int]
    ready_tracks: List[Hashable]
    ready_slots: List[int]
    first_frames: List[int]


class ClosedTrack(NamedTuple):
    """A closed track: its slot, its row count and the trailing rows (row index, frame id) that no window had made final."""
    track: Hashable
    slot: int
    count: int
    rows: List[Tuple[int, int]]


class StreamPlan:
    """Host bookkeeping of `StreamScorer`: track id -> slot (free slots are reused after `close`, lowest first), rows pushed per track,
    the last R frame ids per track, and which tracks have a full window.  Mirrors the device's `count`, so readiness costs no
    device -> host copy."""

    def __init__(self, max_tracks: int, seg_len: int, seg_stride: int = 1) -> None:
        if seg_len not in ops.STREAM_WINDOWS:
            raise ValueError(f"StreamPlan: unsupported window of {seg_len} frames: the stream kernels take {ops.STREAM_WINDOWS}")
        if int(seg_stride) < 1 or int(max_tracks) < 1:
            raise ValueError(f"StreamPlan: seg_stride = {seg_stride}, max_tracks = {max_tracks}")
        self.max_tracks, self.T, self.step = int(max_tracks), int(seg_len), int(seg_stride)
        self.R = ops.stream_rows(self.T, self.step)
        self.reset()

    def reset(self) -> None:
        self.slot_of: Dict[Hashable, int] = {}
        self._free = list(range(self.max_tracks))
        heapq.heapify(self._free)
        self.count = [0] * self.max_tracks
        self.frames = [deque(maxlen=self.R) for _ in range(self.max_tracks)]

    @property
    def live(self) -> List[Hashable]:
        return list(self.slot_of)

    def push(self, frame_id: int, track_ids: Sequence[Hashable]) -> PushPlan:
        ids, frame_id = list(track_ids), int(frame_id)
        if len(set(ids)) != len(ids):
            dup = next(t for i, t in enumerate(ids) if t in ids[:i])
            raise ValueError(f"StreamPlan.push: duplicate track id {dup!r} in one push")
        for t in ids:
            s = self.slot_of.get(t)
            if s is not None and self.frames[s] and frame_id <= self.frames[s][-1]:
                raise ValueError(f"StreamPlan.push: frame id {frame_id} does not increase within track {t!r} "
                                 f"(its last frame is {self.frames[s][-1]})")
        new = sum(1 for t in ids if t not in self.slot_of)
        if new > len(self._free):
            raise ValueError(f"StreamPlan.push: {len(self.slot_of) + new} live tracks, more than max_tracks = {self.max_tracks}; "
                             "close tracks that have ended")
        plan = PushPlan([], [], [], [], [], [])
        for t in ids:
            s = self.slot_of.get(t)
            fresh = s is None
            if fresh:
                s = heapq.heappop(self._free)
                self.slot_of[t] = s
                self.count[s] = 0
                self.frames[s].clear()
            self.count[s] += 1
            self.frames[s].append(frame_id)
            plan.slots.append(s)
            plan.reset.append(int(fresh))
            if self.count[s] >= self.R:
                plan.out_index.append(len(plan.ready_slots))
                plan.ready_tracks.append(t)
                plan.ready_slots.append(s)
                plan.first_frames.append(self.frames[s][0])       # the deque holds rows e - (R - 1) .. e
            else:
                plan.out_index.append(-1)
        return plan

    def close(self, track_ids: Optional[Iterable[Hashable]] = None) -> List[ClosedTrack]:
        """Ends the tracks (all live ones by default) and frees their slots.  The rows that no window has made final are the last
        min(count, R - 1) of each."""
        ids = self.live if track_ids is None else list(track_ids)
        if len(set(ids)) != len(ids):
            raise ValueError("StreamPlan.close: duplicate track id")
        for t in ids:
            if t not in self.slot_of:
                raise ValueError(f"StreamPlan.close: track {t!r} is not live")
        out = []
        for t in ids:
            s = self.slot_of.pop(t)
            n = self.count[s]
            k = min(n, self.R - 1)
            fr = list(self.frames[s])[len(self.frames[s]) - k:] if k else []
            out.append(ClosedTrack(t, s, n, [(n - k + q, f) for q, f in enumerate(fr)]))
            heapq.heappush(self._free, s)
        return out


class StreamOut(NamedTuple):
    """What one `push` (or `close`, whose window fields are empty) hands out.
    tracks / first_frames: the tracks that completed a window and the frame id of each window's first row (`segs_meta[:, 3]`);
    window_scores [K, m] on the device (None at m = 0); final: the (track, frame id) pairs that became final; frame_scores
    [K, len(final)] float64 on the device (None when nothing became final)."""
    tracks: List[Hashable]
    first_frames: List[int]
    window_scores: Optional[torch.Tensor]
    final: List[Tuple[Hashable, int]]
    frame_scores: Optional[torch.Tensor]
    windows: Optional[torch.Tensor] = None          # [K m, 2, T, V]: the batch the stream formed (item k m + j)


def _refusal(lit, what: str = "StreamScorer") -> Optional[str]:
    from .lit import LitVAE
    if isinstance(lit, LitVAE):
        return (f"{what}: LitVAE scores a window by the cosine of a SAMPLED latent, so a replay would not reproduce it; "
                "the one-class encoders and the autoencoder stream")
    if int(getattr(lit.args, "num_coords", 2)) != 2:
        return f"{what}: num_coords = {lit.args.num_coords}; the stream serves the (x, y) layout (num_coords = 2)"
    if lit.model.training:
        return f"{what}: the model is in train mode; scoring is eval-mode arithmetic (call lit.model.eval())"
    return None


class StreamScorer:
    """StreamScorer(lit, scaler, vid_res, max_tracks=256, seg_stride=1, num_transform=1, clip_frames=None)

    lit: a `LitEncoder` (Euclidean, Mahalanobis or Poincare head) or `LitAutoEncoder` in eval mode on the GPU; window length, joint
    layout (`dataset_kp18_format`, `dataset_headless`) come from its args.  scaler: the training run's RobustScaler, or None with
    `normalize_pose` off.  vid_res: (width, height) of the video; None says the rows are normalised already (only the layout applies).
    num_transform: the first K of the dataset's affine transformations (`mats` [K, 3, 3] replaces them).  clip_frames: length of the
    clip vector `clip_scores()` accumulates (max over persons at index frame id - 1), None for none.

    `push` enqueues one pinned non-blocking upload, the push launch, the wrapper's eval scoring of the windows and the frames launch on
    the current stream and never synchronises.  ValueError, naming the reason, for train mode, `LitVAE` and `num_coords != 2`."""

    def __init__(self, lit, scaler, vid_res, max_tracks: int = 256, seg_stride: int = 1, num_transform: int = 1,
                 clip_frames: Optional[int] = None, mats=None) -> None:
        why = _refusal(lit)
        if why:
            raise ValueError(why)
        from .lit import LitAutoEncoder, _joints
        from .utils.dataset import AE_TRANS_MATS
        self.lit, self._ae = lit, isinstance(lit, LitAutoEncoder)
        self.T, self.V = int(lit.args.dataset_seg_len), _joints(lit.args)
        self.plan = StreamPlan(max_tracks, self.T, seg_stride)
        if not ops.stream_ok(self.T, self.V):
            raise ValueError(f"StreamScorer: unsupported (n_frames={self.T}, n_joints={self.V})")
        self.step, self.R, self.M = self.plan.step, self.plan.R, self.plan.max_tracks
        self.flags = (ops.STREAM_KP18 if getattr(lit.args, "dataset_kp18_format", False) else 0) \
            | (ops.STREAM_HEADLESS if getattr(lit.args, "dataset_headless", False) else 0)
        if vid_res is None:
            if scaler is not None:
                raise ValueError("StreamScorer: vid_res = None says the rows are normalised already; a scaler has nothing to do then")
            self.flags |= ops.STREAM_NORMALISED
        self.vid_res = None if vid_res is None else (float(vid_res[0]), float(vid_res[1]))
        dev = self.device = next(lit.model.parameters()).device
        m = np.asarray(AE_TRANS_MATS[:max(1, int(num_transform))] if mats is None else mats, dtype=np.float32).reshape(-1, 3, 3)
        self.K = m.shape[0]
        self.mats = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        self.center = self.scale = None
        if scaler is not None:
            c = getattr(scaler, "center_", None)
            s = getattr(scaler, "scale_", None)
            self.center = torch.from_numpy(np.zeros(N_RAW) if c is None else np.asarray(c, dtype=np.float64).copy()).to(dev)
            self.scale = torch.from_numpy(np.ones(N_RAW) if s is None else np.asarray(s, dtype=np.float64).copy()).to(dev)
        self.ring = torch.zeros(self.M, self.R, 2, self.V, device=dev, dtype=torch.float32)
        self.count = torch.zeros(self.M, device=dev, dtype=torch.int32)
        self.wscore = torch.zeros(self.M, self.K, self.R, device=dev, dtype=torch.float64)
        self.clip = None if clip_frames is None else torch.zeros(self.K, int(clip_frames), device=dev, dtype=torch.float64)
        # one upload per push: raw rows, slots, reset flags, window positions, ready slots and clip indices in one buffer of 4-byte words
        self._cap = self.M * (N_RAW + 5)
        self._pin = [torch.empty(self._cap, dtype=torch.int32).pin_memory() for _ in range(_STAGES)]
        self._pin_np = [p.numpy() for p in self._pin]
        self._busy: List[Optional[torch.cuda.Event]] = [None] * _STAGES
        self._dev = torch.empty(self._cap, device=dev, dtype=torch.int32)
        self._turn = 0

    # ---- the pieces of a push ----------------------------------------------------------------------------------------
    def _stage(self) -> int:
        i = self._turn
        self._turn = (i + 1) % _STAGES
        ev = self._busy[i]
        if ev is not None and not ev.query():       # _STAGES pushes later the upload has long finished; never taken in practice
            ev.synchronize()
        return i

    def _score(self, x: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            if self._ae:
                return self.lit.window_scores_from_batch(x)
            return self.lit.window_scores(self.lit.model(x))

    def push(self, frame_id: int, track_ids: Sequence[Hashable], keypoints) -> StreamOut:
        """The skeletons of one frame: keypoints [n, 17, 2] or [n, 34] (pixel coordinates, zeros = missing joint), one per track id."""
        if self.lit.model.training:
            raise ValueError(_refusal(self.lit, "StreamScorer.push"))
        kp = np.asarray(keypoints.detach().cpu().numpy() if torch.is_tensor(keypoints) else keypoints, dtype=np.float32)
        ids = list(track_ids)
        n = len(ids)
        if kp.size != n * N_RAW or (n and kp.shape[0] != n):
            raise ValueError(f"StreamScorer.push: {n} track ids, keypoints of shape {tuple(kp.shape)}; expected [n, 17, 2] or [n, 34]")
        if n == 0:
            return StreamOut([], [], None, [], None)
        p = self.plan.push(frame_id, ids)
        m = len(p.ready_slots)
        i = self._stage()
        host, a = self._pin_np[i], n * N_RAW
        host[:a].view(np.float32)[:] = kp.reshape(-1)
        host[a:a + n] = p.slots
        host[a + n:a + 2 * n] = p.reset
        host[a + 2 * n:a + 3 * n] = p.out_index
        b = a + 3 * n
        host[b:b + m] = p.ready_slots
        host[b + m:b + 2 * m] = [f - 1 for f in p.first_frames]
        tot = b + 2 * m
        d = self._dev
        d[:tot].copy_(self._pin[i][:tot], non_blocking=True)
        ev = self._busy[i] or torch.cuda.Event()
        ev.record()
        self._busy[i] = ev
        x = ops.stream_push(d[:a].view(torch.float32).view(n, N_RAW), d[a:a + n], self._pin[i][a:a + n], d[a + n:a + 2 * n],
                            d[a + 2 * n:b], self.center, self.scale, self.vid_res, self.flags, self.mats, self.ring, self.count, m,
                            self.T, self.V, self.step)
        if m == 0:
            return StreamOut([], [], None, [], None)
        scores = self._score(x).reshape(-1)
        fm = ops.stream_frames(scores.contiguous(), d[b:b + m], self._pin[i][b:b + m], d[b + m:tot], self.count, self.wscore, self.clip,
                               self.T, self.step)
        return StreamOut(p.ready_tracks, p.first_frames, scores.reshape(self.K, m), list(zip(p.ready_tracks, p.first_frames)), fm, x)

    def close(self, track_ids: Optional[Iterable[Hashable]] = None) -> StreamOut:
        """Ends the tracks (all live ones by default): -> the trailing (track, frame id) rows, final with the windows that exist, and
        their frame scores [K, rows]; all 0 for a track that never filled a window.  The slots are free for new tracks."""
        closed = self.plan.close(track_ids)
        final = [(c.track, f) for c in closed for _, f in c.rows]
        if not final:
            return StreamOut([], [], None, [], None)
        table = torch.tensor([[c.slot for c in closed for _ in c.rows], [r for c in closed for r, _ in c.rows],
                              [f - 1 for c in closed for _, f in c.rows]], dtype=torch.int32).pin_memory()
        dev = table.to(self.device, non_blocking=True)
        fm = ops.stream_close(dev[0], table[0], dev[1], dev[2], self.count, self.wscore, self.clip, self.T, self.step)
        return StreamOut([], [], None, final, fm)

    def clip_scores(self) -> torch.Tensor:
        """[K, clip_frames] float64 on the device: per transformation the max over the persons of the frame scores that are final,
        before smoothing (`eval_utils.frame_scores(..., pad_size=-1)` once every track is closed)."""
        if self.clip is None:
            raise ValueError("StreamScorer.clip_scores: built without clip_frames")
        return self.clip.clone()

    def reset(self, clip_frames: Optional[int] = None) -> None:
        """A new clip: every track is dropped without scores and the clip vector starts from 0 (with a new length, if one is given)."""
        self.plan.reset()
        if clip_frames is not None:
            self.clip = torch.zeros(self.K, int(clip_frames), device=self.device, dtype=torch.float64)
        elif self.clip is not None:
            self.clip.zero_()
