"""Online scoring: live pose tracks in, frame by frame; window scores and per-person frame scores out.

The offline route needs a finished Morais CSV tree (`PoseDatasetRobust` / `PoseFramesRobust`) and a `ScorePlan` of the complete window
table.  Here the same arithmetic runs one frame at a time: `StreamScorer.push` takes the skeletons a tracker found in one frame,
normalises them on the device as `bbox_centre_coordinates` / `scale_robust` / `pose_layout` do, keeps the last R = (T - 1) seg_stride + 1
rows of every track in a ring, scores the window of every track that has one with the wrapper's ordinary eval scoring, and hands out
  * the window scores at once, and
  * the frame score of a (track, frame) R - 1 rows later, when no further window can cover it,
by the rules of `eval_utils.person_frame_scores` -- so replaying a test split reproduces what eval_COSKAD.py computes, bit for bit.
Kernels: csrc/stream.hip.  `StreamPlan` is the host's bookkeeping (slots, row counts, frame ids, readiness) and needs no native library.

`StreamBank` serves many cameras per tick with the launches of one push, and hands out the signal the method is
evaluated on -- the shifted, sigma = 30 Gaussian-smoothed clip score -- at a fixed lag of 120 frames behind the raw score; `BankPlan` is
its host bookkeeping (cameras, the shared slot pool, finality watermarks, what may be emitted).
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
    frame_maps: Optional[torch.Tensor] = None       # maps = True: [K, len(final), V] float64, the per-joint map of every final row
    window_maps: Optional[torch.Tensor] = None      # maps = True: [K m, T, V], the per-joint map of every window (item k m + j)


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


def _maps_refusal(lit, what: str) -> Optional[str]:
    """why `maps = True` does not take this wrapper: the reason its own map call would give, before any push"""
    from .lit import LitAutoEncoder
    if isinstance(lit, LitAutoEncoder):
        why = lit._error_map_refusal()
        return None if why is None else f"{what}: maps = True: window_error_map: {why}"
    from . import attribution
    why = attribution.unsupported_reason(lit)
    return None if why is None else f"{what}: maps = True: window_attribution: {why}"


class _StreamState:
    """What `StreamScorer` and `StreamBank` share: the wrapper and its layout, the transformations, the scaler's columns, the device
    state of the tracks (rings, row counts, score rings) and the pinned staging buffers of the one upload per push."""

    def _setup(self, what, lit, scaler, normalised, max_tracks, seg_stride, num_transform, mats, maps=False) -> None:
        why = _refusal(lit, what) or (_maps_refusal(lit, what) if maps else None)
        if why:
            raise ValueError(why)
        from .lit import LitAutoEncoder, _joints
        from .utils.dataset import AE_TRANS_MATS
        self.lit, self._ae = lit, isinstance(lit, LitAutoEncoder)
        self.T, self.V = int(lit.args.dataset_seg_len), _joints(lit.args)
        self.plan = StreamPlan(max_tracks, self.T, seg_stride)
        if not ops.stream_ok(self.T, self.V):
            raise ValueError(f"{what}: unsupported (n_frames={self.T}, n_joints={self.V})")
        self.step, self.R, self.M = self.plan.step, self.plan.R, self.plan.max_tracks
        self.flags = (ops.STREAM_KP18 if getattr(lit.args, "dataset_kp18_format", False) else 0) \
            | (ops.STREAM_HEADLESS if getattr(lit.args, "dataset_headless", False) else 0)
        if normalised:
            if scaler is not None:
                raise ValueError(f"{what}: vid_res = None says the rows are normalised already; a scaler has nothing to do then")
            self.flags |= ops.STREAM_NORMALISED
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
        # per-joint maps: running fp64 sums and counts per (track, transformation, ring row, joint)
        self.maps = bool(maps)
        self.map_state = ops.stream_maps_state(self.M, self.K, self.T, self.V, self.step, dev) if self.maps else None
        self._turn = 0

    def _staging(self, words: int) -> None:
        self._cap = int(words)
        self._pin = [torch.empty(self._cap, dtype=torch.int32).pin_memory() for _ in range(_STAGES)]
        self._pin_np = [p.numpy() for p in self._pin]
        self._busy: List[Optional[torch.cuda.Event]] = [None] * _STAGES
        self._dev = torch.empty(self._cap, device=self.device, dtype=torch.int32)

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

    def _window_maps(self, x: torch.Tensor) -> torch.Tensor:
        """[K m, T, V]: the wrapper's per-joint map of every window -- the reconstruction error of an autoencoder, the attribution of a
        one-class encoder.  The window scores stay those of `_score`: the map chain's own score is not substituted."""
        if self._ae:
            return self.lit.window_error_map(x)[1].contiguous()
        return self.lit.window_attribution(x)[2].contiguous()


class StreamScorer(_StreamState):
    """StreamScorer(lit, scaler, vid_res, max_tracks=256, seg_stride=1, num_transform=1, clip_frames=None)

    lit: a `LitEncoder` (Euclidean, Mahalanobis or Poincare head) or `LitAutoEncoder` in eval mode on the GPU; window length, joint
    layout (`dataset_kp18_format`, `dataset_headless`) come from its args.  scaler: the training run's RobustScaler, or None with
    `normalize_pose` off.  vid_res: (width, height) of the video; None says the rows are normalised already (only the layout applies).
    num_transform: the first K of the dataset's affine transformations (`mats` [K, 3, 3] replaces them).  clip_frames: length of the
    clip vector `clip_scores()` accumulates (max over persons at index frame id - 1), None for none.  maps: also hand out WHERE a frame
    was anomalous -- `window_maps`, the per-joint map of every window (`window_attribution` of an encoder wrapper,
    `window_error_map` of the autoencoder), and `frame_maps`, the map of every (track, frame) as it becomes final: the mean over its
    covering windows, bit for bit `eval_utils.attribution_frames_device`'s (NaN for a row no window covers).  One map call and one
    launch more per push; ValueError with the map call's own reason for a wrapper it does not take.

    `push` enqueues one pinned non-blocking upload, the push launch, the wrapper's eval scoring of the windows and the frames launch on
    the current stream and never synchronises.  ValueError, naming the reason, for train mode, `LitVAE` and `num_coords != 2`."""

    def __init__(self, lit, scaler, vid_res, max_tracks: int = 256, seg_stride: int = 1, num_transform: int = 1,
                 clip_frames: Optional[int] = None, mats=None, maps: bool = False) -> None:
        self._setup("StreamScorer", lit, scaler, vid_res is None, max_tracks, seg_stride, num_transform, mats, maps)
        self.vid_res = None if vid_res is None else (float(vid_res[0]), float(vid_res[1]))
        self.clip = None if clip_frames is None else torch.zeros(self.K, int(clip_frames), device=self.device, dtype=torch.float64)
        # one upload per push: raw rows, slots, reset flags, window positions, ready slots and clip indices in one buffer of 4-byte words
        self._staging(self.M * (N_RAW + 5))

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
        wmap = fmap = None
        if self.maps:
            wmap = self._window_maps(x)
            fmap = ops.stream_maps(wmap, d[b:b + m], self._pin[i][b:b + m], self.count, self.map_state, self.K, self.T, self.V, self.step)
        return StreamOut(p.ready_tracks, p.first_frames, scores.reshape(self.K, m), list(zip(p.ready_tracks, p.first_frames)), fm, x,
                         fmap, wmap)

    def close(self, track_ids: Optional[Iterable[Hashable]] = None) -> StreamOut:
        """Ends the tracks (all live ones by default): -> the trailing (track, frame id) rows, final with the windows that exist, and
        their frame scores [K, rows]; all 0 for a track that never filled a window (their maps, with `maps`, are NaN then).  The slots
        are free for new tracks."""
        closed = self.plan.close(track_ids)
        final = [(c.track, f) for c in closed for _, f in c.rows]
        if not final:
            return StreamOut([], [], None, [], None)
        table = torch.tensor([[c.slot for c in closed for _ in c.rows], [r for c in closed for r, _ in c.rows],
                              [f - 1 for c in closed for _, f in c.rows]], dtype=torch.int32).pin_memory()
        dev = table.to(self.device, non_blocking=True)
        fm = ops.stream_close(dev[0], table[0], dev[1], dev[2], self.count, self.wscore, self.clip, self.T, self.step)
        fmap = None
        if self.maps:
            fmap = ops.stream_maps_close(dev[0], table[0], dev[1], self.count, self.map_state, self.K, self.T, self.V, self.step)
        return StreamOut([], [], None, final, fm, None, fmap)

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
        if self.map_state is not None:
            self.map_state.zero_()


# ---- many cameras per tick, fixed-lag smoothed scores --------------------------------------------------------------

SMOOTH_LAG = 120                # frames between a raw clip score becoming final and its smoothed score: the filter's radius


def emittable(watermark: int) -> int:
    """How many leading smoothed scores may be handed out at finality watermark W while the clip's end is open: index i once
    W >= i + 121.  The filter's interior needs raw[i + 109] only, but then the value would depend on where the clip later ends (the
    right reflection reaches i + 120); with raw[0 .. i + 120] final it is the offline value for every possible clip end."""
    return max(0, int(watermark) - SMOOTH_LAG)


class _Camera:
    __slots__ = ("res", "n", "offset", "last", "finished", "emitted", "tracks")

    def __init__(self, res, n) -> None:
        self.res, self.n, self.offset = res, n, 0
        self.start(n)

    def start(self, n) -> None:
        self.n = n
        self.last = 0               # the last pushed frame id
        self.finished = None        # the clip length `finish` fixed
        self.emitted = 0            # smoothed scores handed out
        self.tracks: Dict[Hashable, int] = {}       # live track id -> the frame id it was last seen in


class BankTick(NamedTuple):
    """One tick of the bank as the launches need it.  closed: tracks ended before the push (idle, `close`, `finish`), their track field
    (cam, track id); close_clip: the clip index of each of their trailing rows, flat; push: the merged `PushPlan` of all cameras (None
    without detections), ready tracks as (cam, track id); cams: the camera of every detection; clip_index: per ready track;
    smoothed: (cam, first index, count) of the smoothed scores that became emit-able; items: their (offset, n, index) rows."""
    closed: List[ClosedTrack]
    close_clip: List[int]
    push: Optional[PushPlan]
    cams: List[Hashable]
    clip_index: List[int]
    smoothed: List[Tuple[Hashable, int, int]]
    items: List[Tuple[int, int, int]]


class BankPlan:
    """Host bookkeeping of `StreamBank`: the cameras, one `StreamPlan` whose tracks are keyed (cam, track id) -- one shared slot pool --
    the layout of the flat clip buffer (camera c owns [offset, offset + clip_frames)), and per camera the finality watermark

        W = min(last pushed frame id, min over its live tracks of (oldest non-final frame id - 1), clip_frames),

    the number of leading clip entries that can no longer change.  Needs no native library."""

    def __init__(self, cameras, max_tracks: int, seg_len: int, seg_stride: int = 1, smooth: bool = False,
                 idle_close: Optional[int] = None) -> None:
        if not cameras:
            raise ValueError("StreamBank: no cameras")
        if idle_close is not None and int(idle_close) < 0:
            raise ValueError(f"StreamBank: idle_close = {idle_close}")
        self.plan = StreamPlan(max_tracks, seg_len, seg_stride)
        self.smooth, self.idle_close = bool(smooth), None if idle_close is None else int(idle_close)
        self.cams: Dict[Hashable, _Camera] = {}
        for cam, spec in cameras.items():
            spec = dict(spec or {})
            res, n = spec.pop("vid_res", None), spec.pop("clip_frames", None)
            if spec:
                raise ValueError(f"StreamBank: camera {cam!r}: unknown setting {sorted(spec)[0]!r} (vid_res, clip_frames)")
            self.cams[cam] = _Camera(None if res is None else (float(res[0]), float(res[1])), self._length(cam, n))
        if len({c.res is None for c in self.cams.values()}) > 1:
            raise ValueError("StreamBank: cameras with vid_res = None (rows normalised already) and cameras with a resolution in one "
                             "bank; the scaler and the layout are shared, so it is one or the other")
        self._layout()

    def _length(self, cam, n) -> Optional[int]:
        if n is None:
            if self.smooth:
                raise ValueError(f"StreamBank: smooth = True needs clip_frames on every camera; camera {cam!r} has none")
            return None
        if int(n) < 1:
            raise ValueError(f"StreamBank: camera {cam!r}: clip_frames = {n}")
        return int(n)

    def _layout(self) -> None:
        off = 0
        for c in self.cams.values():
            c.offset = off
            off += c.n or 0
        if off > 2 ** 31 - 1:
            raise ValueError(f"StreamBank: {off} clip frames in all; the flat clip buffer is indexed by int32")
        self.total = off

    def _cam(self, cam, what: str) -> _Camera:
        c = self.cams.get(cam)
        if c is None:
            raise ValueError(f"StreamBank.{what}: unknown camera {cam!r}")
        return c

    def clip_index(self, cam, frame_id: int) -> int:
        """offset + frame id - 1, or -1 outside the camera's own segment: the kernels' bound is the flat buffer's length, so only the
        host keeps a camera out of its neighbour's segment"""
        c = self.cams[cam]
        i = int(frame_id) - 1
        return c.offset + i if c.n is not None and 0 <= i < c.n else -1

    def watermark(self, cam) -> int:
        c = self._cam(cam, "watermark")
        w = c.last
        for t in c.tracks:
            s = self.plan.slot_of[(cam, t)]
            fr = self.plan.frames[s]
            w = min(w, (fr[1] if self.plan.count[s] >= self.plan.R else fr[0]) - 1)
        return w if c.n is None else min(w, c.n)

    def _emit(self, cams) -> Tuple[List[Tuple[Hashable, int, int]], List[Tuple[int, int, int]]]:
        smoothed, items = [], []
        if not self.smooth:
            return smoothed, items
        for cam in cams:
            c = self.cams[cam]
            n = c.n if c.finished is None else c.finished
            upto = emittable(self.watermark(cam)) if c.finished is None else n
            if upto > c.emitted:
                smoothed.append((cam, c.emitted, upto - c.emitted))
                items += [(c.offset, n, i) for i in range(c.emitted, upto)]
                c.emitted = upto
        return smoothed, items

    def _close(self, cam, ids) -> Tuple[List[ClosedTrack], List[int]]:
        closed = self.plan.close([(cam, t) for t in ids])
        for t in ids:
            del self.cams[cam].tracks[t]
        return closed, [self.clip_index(cam, f) for c in closed for _, f in c.rows]

    def push(self, batch) -> BankTick:
        """batch: {cam: (frame id, track ids)}.  Everything is checked before anything changes."""
        idle, new, seen = [], 0, 0
        for cam, (f, ids) in batch.items():
            c = self._cam(cam, "push")
            if c.finished is not None:
                raise ValueError(f"StreamBank.push: push after finish: camera {cam!r} has finished its clip; reset(cam) starts the next")
            if int(f) <= c.last:
                raise ValueError(f"StreamBank.push: frame id {int(f)} does not increase on camera {cam!r} (its last frame is {c.last})")
            ids = list(ids)
            if len(set(ids)) != len(ids):
                dup = next(t for i, t in enumerate(ids) if t in ids[:i])
                raise ValueError(f"StreamBank.push: duplicate track id {dup!r} on camera {cam!r} in one push")
            gone = [] if self.idle_close is None else [t for t, last in c.tracks.items() if int(f) - last > self.idle_close]
            idle.append((cam, gone))
            new += sum(1 for t in ids if t not in c.tracks or t in gone)
            seen += len(gone)
        live = len(self.plan.slot_of) - seen + new
        if live > self.plan.max_tracks:
            raise ValueError(f"StreamBank.push: {live} live tracks, more than max_tracks = {self.plan.max_tracks}; close tracks that "
                             "have ended (or set idle_close)")
        closed, close_clip = [], []
        for cam, gone in idle:
            if gone:
                a, b = self._close(cam, gone)
                closed += a
                close_clip += b
        merged, cams, clip_index = PushPlan([], [], [], [], [], []), [], []
        for cam, (f, ids) in batch.items():
            c, ids, f = self.cams[cam], list(ids), int(f)
            c.last = f
            if not ids:
                continue
            p = self.plan.push(f, [(cam, t) for t in ids])
            base = len(merged.ready_slots)
            merged.slots.extend(p.slots)
            merged.reset.extend(p.reset)
            merged.out_index.extend(j + base if j >= 0 else -1 for j in p.out_index)
            merged.ready_tracks.extend(p.ready_tracks)
            merged.ready_slots.extend(p.ready_slots)
            merged.first_frames.extend(p.first_frames)
            cams += [cam] * len(ids)
            clip_index += [self.clip_index(cam, first) for first in p.first_frames]
            for t in ids:
                c.tracks[t] = f
        smoothed, items = self._emit(batch)
        return BankTick(closed, close_clip, merged if cams else None, cams, clip_index, smoothed, items)

    def close(self, cam, track_ids=None) -> BankTick:
        c = self._cam(cam, "close")
        ids = list(c.tracks) if track_ids is None else list(track_ids)
        if len(set(ids)) != len(ids):
            raise ValueError("StreamBank.close: duplicate track id")
        for t in ids:
            if t not in c.tracks:
                raise ValueError(f"StreamBank.close: track {t!r} is not live on camera {cam!r}")
        closed, close_clip = self._close(cam, ids)
        smoothed, items = self._emit([cam])
        return BankTick(closed, close_clip, None, [], [], smoothed, items)

    def finish(self, cam, n_frames: Optional[int] = None) -> BankTick:
        c = self._cam(cam, "finish")
        if c.finished is not None:
            raise ValueError(f"StreamBank.finish: camera {cam!r} has finished its clip already; reset(cam) starts the next")
        if c.n is None:
            if n_frames is not None:
                raise ValueError(f"StreamBank.finish: camera {cam!r} keeps no clip vector (clip_frames = None); n_frames has no meaning")
            n = 0
        else:
            n = c.n if n_frames is None else int(n_frames)
            if not max(1, min(c.last, c.n)) <= n <= c.n:
                raise ValueError(f"StreamBank.finish: n_frames = {n} on camera {cam!r}: between its last pushed frame id "
                                 f"({min(c.last, c.n)}) and clip_frames = {c.n}")
        closed, close_clip = self._close(cam, list(c.tracks))
        c.finished = n
        smoothed, items = self._emit([cam])
        return BankTick(closed, close_clip, None, [], [], smoothed, items)

    def reset(self, cam, clip_frames: Optional[int] = None) -> bool:
        """A new clip on the camera: its tracks are dropped without scores.  -> whether the flat buffer's layout changed."""
        c = self._cam(cam, "reset")
        n = c.n if clip_frames is None else self._length(cam, clip_frames)
        self.plan.close([(cam, t) for t in c.tracks])
        moved = n != c.n
        c.start(n)
        if moved:
            self._layout()
        return moved


class BankOut(NamedTuple):
    """What one `StreamBank.push` (or `close` / `finish`, whose window fields are empty) hands out: `StreamOut`'s fields with tracks as
    (cam, track id), and the smoothed scores that became emit-able -- smoothed: (cam, first index, count) in the order of the columns of
    smoothed_scores [K, sum of counts] (per transformation) and smoothed_mean [sum of counts] (their mean), float64 on the device, None
    when nothing was emitted."""
    tracks: List[Hashable]
    first_frames: List[int]
    window_scores: Optional[torch.Tensor]
    final: List[Tuple[Hashable, int]]
    frame_scores: Optional[torch.Tensor]
    windows: Optional[torch.Tensor] = None
    smoothed: Sequence[Tuple[Hashable, int, int]] = ()
    smoothed_scores: Optional[torch.Tensor] = None
    smoothed_mean: Optional[torch.Tensor] = None
    frame_maps: Optional[torch.Tensor] = None       # maps = True: [K, len(final), V] float64
    window_maps: Optional[torch.Tensor] = None      # maps = True: [K m, T, V]


class StreamBank(_StreamState):
    """StreamBank(lit, scaler, cameras, max_tracks=1024, seg_stride=1, num_transform=1, mats=None, smooth=False, idle_close=None)

    cameras: {camera id: dict(vid_res=(w, h) | None, clip_frames=n | None)}.  The model, scaler, layout, window, stride and
    transformations are shared (as `StreamScorer` takes them); the resolution and the clip vector are per camera.

    `push({cam: (frame_id, track_ids, keypoints)})` serves any number of cameras, each with its own frame id, with ONE pinned
    non-blocking upload, one push launch, one call of the wrapper's eval scoring on the ready windows of all cameras and one frames
    launch -- plus a close launch on ticks where `idle_close` ended tracks, and with `smooth` one smoothing launch on ticks where a
    smoothed score became emit-able.  Nothing synchronises, and the number of library calls does not depend on the number of cameras.
    smooth: hand out the shifted, Gaussian-smoothed clip score (what the offline evaluation thresholds) 120 frames behind the raw one;
    `finish(cam)` emits the clip's tail.  idle_close = N closes, at the start of a push, the tracks of a pushed camera not seen for more
    than N of its frame ids (a lost track would hold the camera's watermark back for ever).  maps: as `StreamScorer`'s -- one map call
    on the ready windows of all cameras and ONE maps launch per tick (plus one beside the close launch on ticks that close tracks); the
    map state is indexed by slot, as the score ring is, and keyed on the row count, so `reset(cam)` has nothing to clear."""

    def __init__(self, lit, scaler, cameras, max_tracks: int = 1024, seg_stride: int = 1, num_transform: int = 1, mats=None,
                 smooth: bool = False, idle_close: Optional[int] = None, maps: bool = False) -> None:
        why = _refusal(lit, "StreamBank")
        if why:
            raise ValueError(why)
        self.bank = BankPlan(cameras, max_tracks, int(lit.args.dataset_seg_len), seg_stride, smooth, idle_close)
        normalised = next(iter(self.bank.cams.values())).res is None
        self._setup("StreamBank", lit, scaler, normalised, max_tracks, seg_stride, num_transform, mats, maps)
        self.plan = self.bank.plan
        self.smooth = self.bank.smooth
        self.clip = self._new_clip()
        if self.smooth:
            from .utils.score_plan import gaussian_taps
            self.taps = torch.from_numpy(gaussian_taps()).to(self.device)
        self._staging(self._words())

    def _new_clip(self) -> Optional[torch.Tensor]:
        return torch.zeros(self.K, self.bank.total, device=self.device, dtype=torch.float64) if self.bank.total else None

    def _words(self) -> int:
        # raw rows, slots, reset flags, window positions, resolutions, ready slots, clip indices | trailing rows of closed tracks | items
        return self.M * (N_RAW + 7) + 3 * self.M * (self.R - 1) + (3 * self.bank.total if self.smooth else 0)

    # ---- one upload, then the launches, for whatever a tick holds ----------------------------------------------------------------
    def _run(self, tick: BankTick, kp: Optional[np.ndarray]) -> BankOut:
        p = tick.push
        n, m = (len(p.slots), len(p.ready_slots)) if p is not None else (0, 0)
        r, s = len(tick.close_clip), len(tick.items)
        if n + r + s == 0:
            return BankOut([], [], None, [], None)
        i = self._stage()
        host, pin, d = self._pin_np[i], self._pin[i], self._dev
        a = n * N_RAW
        b = a + 5 * n                       # slots, reset, out_index, res
        c = b + 2 * m                       # ready slots, clip indices
        e = c + 3 * r                       # row slots, row indices, clip indices of the closed tracks' trailing rows
        tot = e + 3 * s                     # items
        if n:
            host[:a].view(np.float32)[:] = kp.reshape(-1)
            host[a:a + n] = p.slots
            host[a + n:a + 2 * n] = p.reset
            host[a + 2 * n:a + 3 * n] = p.out_index
            if not self.flags & ops.STREAM_NORMALISED:
                host[a + 3 * n:b].view(np.float32)[:] = np.asarray([self.bank.cams[cam].res for cam in tick.cams], np.float32).reshape(-1)
            host[b:b + m] = p.ready_slots
            host[b + m:c] = tick.clip_index
        if r:
            host[c:c + r] = [t.slot for t in tick.closed for _ in t.rows]
            host[c + r:c + 2 * r] = [q for t in tick.closed for q, _ in t.rows]
            host[c + 2 * r:e] = tick.close_clip
        if s:
            host[e:tot] = np.asarray(tick.items, np.int32).reshape(-1)
        d[:tot].copy_(pin[:tot], non_blocking=True)
        ev = self._busy[i] or torch.cuda.Event()
        ev.record()
        self._busy[i] = ev
        final, parts, mparts, wmap = [], [], [], None
        if r:       # before the push launch: a freed slot may start a new track in this very tick
            parts.append(ops.stream_close(d[c:c + r], pin[c:c + r], d[c + r:c + 2 * r], d[c + 2 * r:e], self.count, self.wscore, self.clip,
                                          self.T, self.step))
            if self.maps:
                mparts.append(ops.stream_maps_close(d[c:c + r], pin[c:c + r], d[c + r:c + 2 * r], self.count, self.map_state, self.K,
                                                    self.T, self.V, self.step))
            final += [(t.track, f) for t in tick.closed for _, f in t.rows]
        scores = x = None
        if n:
            norm = bool(self.flags & ops.STREAM_NORMALISED)
            x = ops.stream_push_cams(d[:a].view(torch.float32).view(n, N_RAW), d[a:a + n], pin[a:a + n], d[a + n:a + 2 * n],
                                     d[a + 2 * n:a + 3 * n], self.center, self.scale,
                                     None if norm else d[a + 3 * n:b].view(torch.float32).view(n, 2),
                                     None if norm else pin[a + 3 * n:b].view(torch.float32), self.flags, self.mats, self.ring,
                                     self.count, m, self.T, self.V, self.step)
        if m:
            scores = self._score(x).reshape(-1)
            parts.append(ops.stream_frames(scores.contiguous(), d[b:b + m], pin[b:b + m], d[b + m:c], self.count, self.wscore, self.clip,
                                           self.T, self.step))
            final += list(zip(p.ready_tracks, p.first_frames))
            if self.maps:
                wmap = self._window_maps(x)
                mparts.append(ops.stream_maps(wmap, d[b:b + m], pin[b:b + m], self.count, self.map_state, self.K, self.T, self.V,
                                              self.step))
        per_t = mean = None
        if s:
            per_t, mean = ops.stream_smooth(self.clip, d[e:tot].view(s, 3), pin[e:tot], self.taps)
        fm = None if not parts else parts[0] if len(parts) == 1 else torch.cat(parts, 1)
        fmap = None if not mparts else mparts[0] if len(mparts) == 1 else torch.cat(mparts, 1)
        return BankOut(list(p.ready_tracks) if m else [], list(p.first_frames) if m else [], scores.reshape(self.K, m) if m else None,
                       final, fm, x, tick.smoothed, per_t, mean, fmap, wmap)

    def push(self, batch) -> BankOut:
        """batch: {cam: (frame_id, track_ids, keypoints)}, keypoints [n, 17, 2] or [n, 34] per camera (pixel coordinates, zeros =
        missing joint); a camera whose frame shows nobody is pushed with no track ids, so that its watermark moves on."""
        if self.lit.model.training:
            raise ValueError(_refusal(self.lit, "StreamBank.push"))
        rows, ids = [], {}
        for cam, (f, tids, keypoints) in batch.items():
            kp = np.asarray(keypoints.detach().cpu().numpy() if torch.is_tensor(keypoints) else keypoints, dtype=np.float32)
            tids = list(tids)
            if kp.size != len(tids) * N_RAW or (tids and kp.shape[0] != len(tids)):
                raise ValueError(f"StreamBank.push: camera {cam!r}: {len(tids)} track ids, keypoints of shape {tuple(kp.shape)}; "
                                 "expected [n, 17, 2] or [n, 34]")
            ids[cam] = (f, tids)
            if tids:
                rows.append(kp.reshape(len(tids), N_RAW))
        return self._run(self.bank.push(ids), np.concatenate(rows) if rows else None)

    def close(self, cam, track_ids: Optional[Iterable[Hashable]] = None) -> BankOut:
        """Ends tracks of a camera (all its live ones by default), as `StreamScorer.close`; with `smooth` the watermark may move."""
        return self._run(self.bank.close(cam, track_ids), None)

    def finish(self, cam, n_frames: Optional[int] = None) -> BankOut:
        """The camera's clip is over: closes its live tracks, fixes the clip length n <= clip_frames (clip_frames by default) and, with
        `smooth`, emits every smoothed score not yet emitted, now with the right-hand reflection at n.  `reset(cam)` before the camera is
        pushed again."""
        return self._run(self.bank.finish(cam, n_frames), None)

    def watermark(self, cam) -> int:
        return self.bank.watermark(cam)

    def clip_scores(self, cam) -> torch.Tensor:
        """[K, clip_frames] float64 on the device ([K, n] after `finish` fixed n): the camera's segment of the flat clip buffer, before
        smoothing"""
        c = self.bank._cam(cam, "clip_scores")
        if c.n is None:
            raise ValueError(f"StreamBank.clip_scores: camera {cam!r} was built without clip_frames")
        return self.clip[:, c.offset:c.offset + (c.n if c.finished is None else c.finished)].clone()

    def reset(self, cam, clip_frames: Optional[int] = None) -> None:
        """A new clip on the camera: its tracks are dropped without scores, its clip vector starts from 0 (with a new length, if one is
        given: the other cameras' segments move inside a new flat buffer)."""
        old = {k: (c.offset, c.n) for k, c in self.bank.cams.items()}
        if self.bank.reset(cam, clip_frames):
            clip = self._new_clip()
            for k, c in self.bank.cams.items():
                if k != cam and c.n:
                    clip[:, c.offset:c.offset + c.n] = self.clip[:, old[k][0]:old[k][0] + c.n]
            self.clip = clip
            if self._words() > self._cap:
                self._staging(self._words())
        elif self.bank.cams[cam].n:
            c = self.bank.cams[cam]
            self.clip[:, c.offset:c.offset + c.n].zero_()
