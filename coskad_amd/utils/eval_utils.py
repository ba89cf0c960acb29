"""Window -> frame -> clip anomaly scoring (mirror of the reference's utils/eval_utils.py + the scoring loops of
eval_COSKAD.py:140-253 and the wrappers' post_processing), vectorised.

The reference walks transformations x clips x persons in Python and scatters one window at a time
(eval_utils.py:69-74).  Here the per-window scores come from the HIP head kernels (coskad_amd.ops.mse_head /
poincare_head: MSELoss(reduction='none')(c,z).mean(-1) resp. dist(c, zh)), and the aggregation is ONE segmented
reduction keyed on (transformation, scene, clip, person, frame) with torch index ops on whatever device the
scores live on.  Smoothing and AUC use the same scipy / sklearn calls as the reference (eval_utils.py:206,218).

`score_dataset_device` (utils/score_plan.py) is the same scoring on the device: index tables derived once from the window table
(`ScorePlan`) and the kernels of csrc/score_frames.hip per call; `score_dataset` below stays the host route and the yardstick.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
from scipy.ndimage import gaussian_filter1d
from sklearn.metrics import roc_auc_score, roc_curve

from .score_plan import ScorePlan, auc_device, gaussian_taps, score_dataset_device   # noqa: F401  (the device route of score_dataset)
from .score_plan import ScoreReport, check_segments, report_from_frame_scores, score_report_device   # noqa: F401  (the report)


def score_process(score: np.ndarray, win_size: int = 50, dataname: str = 'STC', use_scaler: bool = False) -> np.ndarray:
    """Shift by 11 frames and Gaussian-smooth with sigma 30 (reference eval_utils.py:200-207)."""
    scores_shifted = np.zeros_like(score)
    shift = 8 + (8 // 2) - 1
    scores_shifted[shift:] = score[:-shift]
    return gaussian_filter1d(scores_shifted, 30)


def filter_vectors_by_cond(vecs, cond):
    """reference eval_utils.py:168-172."""
    return [v[cond] for v in vecs]


def zero_runs(score: np.ndarray, n: int):
    """Inclusive (first, last) index pairs of the maximal runs of exactly-zero entries among frames 0..n-1
    (the `ranges` helper of the reference, eval_utils.py:210-214, applied to the set of zero frames)."""
    z = np.zeros(n + 2, dtype=bool)
    z[1:n + 1] = score[:n] == 0
    starts = np.nonzero(z[1:n + 1] & ~z[0:n])[0]
    ends = np.nonzero(z[1:n + 1] & ~z[2:n + 2])[0]
    return list(zip(starts.tolist(), ends.tolist()))


def pad_scores(score: np.ndarray, gt: np.ndarray, pad_size: int) -> np.ndarray:
    """Widen every interval in which a person is absent (score exactly 0) by `pad_size` frames on the sides that
    touch a presence interval, zeroing the scores there (reference eval_utils.py:232-248; in place, like the
    reference).  Quirks kept: absence is looked for among frames 0..len(gt)-2 only, an all-absent person is left
    alone, and the zeroed range excludes its upper end."""
    n = len(gt)
    last = n - 2
    for a, b in zero_runs(score, n - 1):
        if a == 0 and b == last:
            continue
        lo = a if a == 0 else max(a - pad_size, 0)
        hi = b if (b == last and a != 0) else min(b + pad_size, n)
        score[lo:hi] = 0
    return score


def person_frame_scores(window_scores: torch.Tensor, trans: torch.Tensor, meta: torch.Tensor, frames: torch.Tensor,
                        fmax: int):
    """Segmented mean of the window scores covering each frame, keyed on (transformation, scene, clip, person):
    -> (keys [P,4] int64 (cpu), mean [P,fmax] float64 on the scores' device).  A window whose score is exactly 0
    counts as missing (the reference's `== 0.0 -> NaN` + nanmean, eval_COSKAD.py:201-203); frames nobody covers are 0."""
    dev = window_scores.device
    s = window_scores.reshape(-1).to(torch.float64)
    N, T = frames.shape
    trans, meta, frames = trans.to(dev).long(), meta.to(dev).long(), frames.to(dev).long()
    key_p = torch.stack([trans, meta[:, 0], meta[:, 1], meta[:, 2]], 1)
    uniq_p, pid = torch.unique(key_p, dim=0, return_inverse=True)
    idx = (pid[:, None] * fmax + (frames - 1)).reshape(-1)               # `frames - 1`: eval_utils.py:72
    w = s[:, None].expand(N, T).reshape(-1)
    valid = (w != 0).to(torch.float64)
    ssum = torch.zeros(uniq_p.shape[0] * fmax, dtype=torch.float64, device=dev).index_add_(0, idx, w * valid)
    cnt = torch.zeros_like(ssum).index_add_(0, idx, valid)
    mean = torch.where(cnt > 0, ssum / cnt.clamp_min(1), torch.zeros_like(ssum)).reshape(-1, fmax)
    return uniq_p.cpu(), mean


def frame_scores(window_scores: torch.Tensor, trans: torch.Tensor, meta: torch.Tensor, frames: torch.Tensor,
                 clip_lengths: Dict[Tuple[int, int], int], num_transform: int, pad_size: int = -1,
                 gts: Optional[Dict[Tuple[int, int], np.ndarray]] = None):
    """-> dict {(t, scene, clip): np.ndarray[n_frames]} of per-frame clip scores BEFORE smoothing:
    mean over the windows covering a frame, optional absence padding per person (`pad_size != -1`,
    eval_COSKAD.py:205-206), then max over persons (eval_COSKAD.py:201-211)."""
    fmax = int(max(clip_lengths.values()))
    uniq_p, mean = person_frame_scores(window_scores, trans, meta, frames, fmax)
    dev = mean.device
    uniq_c, cid_of_p = torch.unique(uniq_p[:, :3], dim=0, return_inverse=True)
    if pad_size != -1:
        # per-person interval surgery on the host (a few thousand short vectors), then the max over persons
        m = mean.cpu().numpy()
        for i, (t, sc, cl, _) in enumerate(uniq_p.tolist()):
            n = clip_lengths.get((sc, cl))
            if n is not None:
                ref_gt = gts[(sc, cl)] if gts is not None else np.zeros(n)
                m[i, :n] = pad_scores(m[i, :n].copy(), ref_gt, pad_size)
        mean = torch.from_numpy(m).to(dev)
    clip = torch.full((uniq_c.shape[0], fmax), -float("inf"), dtype=torch.float64, device=dev)
    clip = clip.scatter_reduce(0, cid_of_p.to(dev)[:, None].expand(-1, fmax), mean, reduce="amax", include_self=True)
    clip = clip.cpu().numpy()
    out = {}
    for i, (t, sc, cl) in enumerate(uniq_c.tolist()):
        n = clip_lengths.get((sc, cl))
        if n is not None and t < num_transform:
            out[(t, sc, cl)] = clip[i, :n]
    return out


def score_dataset(window_scores, trans, meta, frames, gts: Dict[Tuple[int, int], np.ndarray], num_transform: int,
                  smoothing: int = 50, dataname: str = 'UBnormal', pad_size: int = -1,
                  hr_masks: Optional[Dict[Tuple[int, int], np.ndarray]] = None):
    """Full scoring: -> (final AUC, {t: smoothed score vector}, concatenated gt).
    gts: {(scene, clip): frame mask}, clips are concatenated in sorted key order (sorted(os.listdir(gt_path))).
    pad_size: eval_COSKAD.py:205-206 (`-1` = off).  hr_masks: {(scene, clip): boolean frame selector} of the
    human-related subsets (utils/model_utils.py:149-161): applied to the clip score and its ground truth before
    smoothing (eval_COSKAD.py:213-215)."""
    lengths = {k: int(v.shape[0]) for k, v in gts.items()}
    fs = frame_scores(torch.as_tensor(window_scores), torch.as_tensor(trans), torch.as_tensor(meta),
                      torch.as_tensor(frames), lengths, num_transform, pad_size=pad_size, gts=gts)
    keys = sorted(gts.keys())
    hr_masks = hr_masks or {}
    per_t = {}
    for t in range(num_transform):
        parts = []
        for k in keys:
            raw = fs.get((t, k[0], k[1]))
            if raw is None:
                raw = np.zeros(lengths[k])          # a clip without detections scores 0 everywhere
            if k in hr_masks:
                raw = raw[hr_masks[k]]
            parts.append(score_process(raw, win_size=smoothing, dataname=dataname, use_scaler=False))
        per_t[t] = np.concatenate(parts)
    gt = np.concatenate([gts[k][hr_masks[k]] if k in hr_masks else gts[k] for k in keys])
    pds = np.mean(np.stack(list(per_t.values()), 0), 0)
    return roc_auc_score(gt, pds), per_t, gt


def hr_masks_from_dir(pattern: str) -> Dict[Tuple[int, int], np.ndarray]:
    """{(scene, clip): boolean mask} from `<scene>_<clip>.npy` files matching a glob (utils/model_utils.py:149-161)."""
    import glob
    import os
    out = {}
    for path in glob.glob(pattern):
        sc, cl = (int(v) for v in os.path.basename(path).split('.')[0].split('_')[:2])
        out[(sc, cl)] = np.load(path)
    return out


def rec_and_hy_window_scores(x: torch.Tensor, x_rec: torch.Tensor, z: torch.Tensor, c: torch.Tensor,
                             rec_loss_weight: float = 0.2, loss_type: str = 'rec') -> torch.Tensor:
    """Per-window score of the autoencoder wrapper (eval_utils.py:77-106): 'rec' = mean squared reconstruction
    error over (T, V, C), 'hyp' = mean squared distance of the latent to the centre, 'rec+hyp' = rec / weight + hyp.
    The 'hyp' part runs on the HIP head kernel when the latents live on the GPU."""
    B = x.shape[0]
    rec = ((x_rec - x) ** 2).reshape(B, -1).mean(-1)
    return rec_and_hy_from_rec(rec, z, c, rec_loss_weight, loss_type)


def rec_and_hy_from_rec(rec: torch.Tensor, z: torch.Tensor, c: torch.Tensor, rec_loss_weight: float = 0.2,
                        loss_type: str = 'rec') -> torch.Tensor:
    """rec_and_hy_window_scores from the per-window reconstruction error `rec` [B] itself (STSAE.reconstruction_scores forms it
    without a reconstruction in memory); `rec` may be None for 'hyp', which does not read it."""
    if loss_type == 'rec':
        return rec
    from .. import ops
    if z.is_cuda and z.shape[1] <= ops.BTLNK_LMAX:   # the head kernels take latents up to 512; wider ones: torch expression
        _, _, hyp = ops.mse_head(z.contiguous().float(), c.float().contiguous(), need_grad=False, need_score=True)
    else:
        hyp = ((z - c) ** 2).mean(-1)
    if loss_type == 'hyp':
        return hyp
    if loss_type == 'rec+hyp':
        return rec / rec_loss_weight + hyp
    raise ValueError(f"unknown loss_type {loss_type}")


def eval_loss_type(rec_loss_weight: float) -> str:
    """eval_COSKAD.py:58-66: the evaluation script derives the score type from its rec_loss_weight constant."""
    if rec_loss_weight == 0:
        return 'hyp'
    return 'rec' if rec_loss_weight > 100 else 'rec+hyp'


def ROC(y_test, y_pred):
    """AUC (reference eval_utils.py:216-230 without the matplotlib plot)."""
    return roc_auc_score(y_test, y_pred)


# ---- the evaluation report on the host: the reference's loops (eval_COSKAD.py:222-242), the yardstick of
# ---- score_plan.score_report_device

def roc_crossing_thresholds(y, s) -> np.ndarray:
    """The first return value of the reference's ROC() (eval_utils.py:217-219,230): the thresholds of sklearn's roc_curve (its
    defaults, so drop_intermediate=True) at which tpr - (1 - fpr) changes sign; one or two values, the first may be inf.  Empty for a
    single-class ground truth, where the curve is not defined."""
    y = np.asarray(y) != 0
    if y.all() or not y.any():
        return np.zeros(0, dtype=np.float64)
    fpr, tpr, tr = roc_curve(y, np.asarray(s, dtype=np.float64))
    idx = np.argwhere(np.diff(np.sign(tpr - (1 - fpr)))).flatten()
    return np.asarray(tr[idx], dtype=np.float64)


def _auc_or_nan(y: np.ndarray, s: np.ndarray) -> float:
    """roc_auc_score, NaN where it is undefined: one class or no frame (sklearn raises there or, from 1.6 on, warns and returns NaN;
    the reference swallows the exception and leaves the clip out of its average)."""
    if y.size == 0 or y.all() or not y.any():
        return float("nan")
    return float(roc_auc_score(y, s))


def clip_segments(gts: Dict[Tuple[int, int], np.ndarray], hr_masks: Optional[Dict[Tuple[int, int], np.ndarray]] = None):
    """-> (sorted clip keys, segments [C, 2]): each clip's [start, end) in `score_dataset`'s concatenated, human-related-compacted
    vectors."""
    keys = sorted(gts.keys())
    hr_masks = hr_masks or {}
    n = [int(np.asarray(gts[k])[hr_masks[k]].shape[0]) if k in hr_masks else int(np.asarray(gts[k]).shape[0]) for k in keys]
    ends = np.cumsum(n, dtype=np.int64)
    return keys, np.stack([ends - n, ends], 1).reshape(-1, 2)


def score_report(per_t, gt, segments, clip_keys) -> ScoreReport:
    """The report as the reference forms it: one roc_auc_score per (transformation, clip), one roc_curve per transformation, in Python
    loops.  per_t: {t: scores [F]} as `score_dataset` returns it, or an array [nt, F]; gt [F] (non-zero = positive); segments [C, 2]."""
    rows = np.stack([np.asarray(per_t[t], dtype=np.float64) for t in sorted(per_t)], 0) if isinstance(per_t, dict) \
        else np.asarray(_host_array(per_t), dtype=np.float64)
    nt, F = rows.shape
    y = np.asarray(gt).reshape(-1) != 0
    seg = check_segments(segments, F)
    if y.shape[0] != F or seg.shape[0] != len(clip_keys):
        raise ValueError(f"score_report: {F} frames, gt of {y.shape[0]}, {seg.shape[0]} segments for {len(clip_keys)} clips")
    pds = np.mean(rows, 0)
    clip_auc = np.array([[_auc_or_nan(y[a:b], rows[t, a:b]) for a, b in seg.tolist()] for t in range(nt)]).reshape(nt, -1)
    return ScoreReport(auc=roc_auc_score(y, pds), auc_t=[roc_auc_score(y, rows[t]) for t in range(nt)],
                       thresholds_t=[roc_crossing_thresholds(y, rows[t]) for t in range(nt)], clip_auc=clip_auc,
                       clip_auc_final=[_auc_or_nan(y[a:b], pds[a:b]) for a, b in seg.tolist()], clip_keys=clip_keys,
                       n_pos=[int(y[a:b].sum()) for a, b in seg.tolist()], n_neg=[int((~y[a:b]).sum()) for a, b in seg.tolist()],
                       segments=seg, frame_scores=pds)


def _host_array(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


# ---- attribution maps: windows -> person frames -> per-clip files ----

def _entry_frames(plan: ScorePlan) -> np.ndarray:
    """[row_ptr[P]] int64: the frame NUMBER (as the window table's `frames` counts them: from 1) of every row of the person x frame
    vector"""
    rp = plan.row_ptr.cpu().numpy().astype(np.int64)
    return np.arange(int(rp[-1]), dtype=np.int64) - np.repeat(rp[:-1], np.diff(rp)) + 1


def attribution_frames(attr, frames, plan: ScorePlan) -> np.ndarray:
    """The yardstick of `attribution_frames_device`, as numpy loops: attr [N, T, V] per-window maps, frames [N, T] the window table's
    frame numbers -> [row_ptr[P], V] float64: for every person-frame the mean over its covering windows (the plan's window CSR, in
    ascending order) of the row attr[w, t] with frames[w, t] == that frame; NaN where no window holds it.  fp64 sums."""
    a, fr = np.asarray(_host_array(attr)), np.asarray(_host_array(frames)).astype(np.int64)
    if a.ndim != 3 or fr.shape != a.shape[:2] or a.shape[0] != plan.N:
        raise ValueError(f"attribution_frames: attr {a.shape}, frames {fr.shape} for a plan of {plan.N} windows")
    wp, wi = plan.win_ptr.cpu().numpy(), plan.win_idx.cpu().numpy()
    ef = _entry_frames(plan)
    out = np.full((ef.shape[0], a.shape[2]), np.nan, dtype=np.float64)
    for e in range(ef.shape[0]):
        total, cnt = np.zeros(a.shape[2], dtype=np.float64), 0
        for w in wi[wp[e]:wp[e + 1]]:
            hit = np.nonzero(fr[w] == ef[e])[0]
            if hit.size:
                total = total + a[w, hit[0]].astype(np.float64)
                cnt += 1
        if cnt:
            out[e] = total / float(cnt)
    return out


def attribution_frames_device(attr: torch.Tensor, frames: torch.Tensor, plan: ScorePlan) -> torch.Tensor:
    """`attribution_frames` on the device (csrc/attribution_frames.hip: one deterministic launch, fp64 sums in the same order, no
    atomics): attr [N, T, V] float32 on the GPU -> [row_ptr[P], V] float64 there."""
    from .. import _lib, ops
    if not attr.is_cuda:
        raise _lib.CoskadHipError(f"attribution_frames_device: expected the maps on the GPU, got device {attr.device}; no CPU fallback "
                                  "(`attribution_frames` is the host route)")
    if attr.dim() != 3 or tuple(frames.shape) != tuple(attr.shape[:2]) or attr.shape[0] != plan.N:
        raise ValueError(f"attribution_frames_device: attr {tuple(attr.shape)}, frames {tuple(frames.shape)} for a plan of {plan.N} "
                         "windows")
    if attr.device != plan.win_ptr.device:
        raise ValueError(f"attribution_frames_device: maps on {attr.device}, plan on {plan.win_ptr.device}")
    if plan.n_persons == 0:
        return torch.empty(0, attr.shape[2], dtype=torch.float64, device=attr.device)
    ef = torch.from_numpy(_entry_frames(plan)).to(torch.int32).to(attr.device)
    return ops.attribution_frames(attr.float().contiguous(), frames.to(attr.device, torch.int32).contiguous(), plan.win_ptr,
                                  plan.win_idx, ef)


def save_attribution(directory: str, maps, plan: ScorePlan, suffix: str = "attribution") -> None:
    """Per clip of the plan `<scene>_<clip>_attribution.npy` [persons, frames, V] float32 -- the person-frame maps [row_ptr[P], V] of
    `attribution_frames(_device)` averaged over the transformations, NaN where the person is absent -- and `<scene>_<clip>_persons.npy`,
    the person ids of its rows (a clip nobody appears in gets arrays with no person).  `suffix`: the map file's name behind
    `<scene>_<clip>_` (attribution.dataset_error_maps writes `error_map`)."""
    if suffix == "persons":
        raise ValueError("save_attribution: the suffix `persons` is the name of the person-id file")
    import os
    os.makedirs(directory, exist_ok=True)
    m = np.asarray(_host_array(maps), dtype=np.float64)
    rp = plan.row_ptr.cpu().numpy().astype(np.int64)
    V = m.shape[1] if m.ndim == 2 else 0
    for c, (sc, cl) in enumerate(plan.clip_keys):
        rows = np.nonzero(plan.person_clip == c)[0]
        ids = np.unique(plan.person_keys[rows, 3]) if rows.size else np.zeros(0, dtype=np.int64)
        n = int(plan.person_n[rows[0]]) if rows.size else 0
        total, cnt = np.zeros((ids.shape[0], n, V)), np.zeros((ids.shape[0], n, V))
        for p in rows:
            k = int(np.searchsorted(ids, plan.person_keys[p, 3]))
            blk = m[rp[p]:rp[p + 1]]
            ok = ~np.isnan(blk)
            total[k] += np.where(ok, blk, 0.0)
            cnt[k] += ok
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.where(cnt > 0, total / cnt, np.nan).astype(np.float32)
        np.save(os.path.join(directory, f"{sc}_{cl}_{suffix}.npy"), out)
        np.save(os.path.join(directory, f"{sc}_{cl}_persons.npy"), ids.astype(np.int64))
