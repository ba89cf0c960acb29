"""Thin, checked wrappers: torch CUDA tensors -> C-ABI calls (include/coskad_hip.h).

Every wrapper validates device / dtype / contiguity / shape on the host before a kernel
sees a pointer, enqueues on torch's current stream and never synchronises.  Arguments go to
the library as plain values (tensors, None, Python numbers): _lib binds every entry point to
its prototype in the header, which converts them and rejects a wrong count or type.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import call

Tensor = torch.Tensor


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: Optional[Tensor], name: str, shape=None, dtype=torch.float32, optional=False) -> None:
    if t is None:
        if optional:
            return
        raise ValueError(f"{name}: tensor required")
    if not t.is_cuda:
        raise _lib.CoskadHipError(f"{name}: expected a CUDA (ROCm) tensor, got device {t.device}; "
                                  "the COSKAD hot path runs only on the HIP extension (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


# A wrapper that hands the library a pointer to module state the kernel will write (a parameter, a BatchNorm running buffer or
# num_batches_tracked) calls note_raw_write(); any cache of tensors derived from module state puts raw_write_epoch() in its key.
_raw_write_epoch = 0


def note_raw_write() -> None:
    global _raw_write_epoch
    _raw_write_epoch += 1


def raw_write_epoch() -> int:
    return _raw_write_epoch


def _bytes(t: Tensor) -> int:
    return t.numel() * t.element_size()


def cop(co: int) -> int:
    return (co + 15) // 16 * 16


WINDOW_LENGTHS = (8, 16, 24)        # window lengths beside 12 that have mixing kernels (csrc/gcn_window.hip)
JOINT_LAYOUTS = (14, 17, 18, 25)    # joint counts every (T, V) kernel is instantiated for


def window_ok(T: int, V: int) -> bool:
    """Host arithmetic of `coskad_window_ok`: (T, V) has mixing kernels only, so a layer of that window length takes the composed
    path.  False at T = 12, the tile kernels' geometry.  Restated here so that building a model needs no native library;
    tests/test_window_host.py holds the two in agreement."""
    return T in WINDOW_LENGTHS and V in JOINT_LAYOUTS


TRAIN_WINDOW_JOINTS = (17, 25)          # joint layouts, input and output widths of the stored-Z training kernels at those window
TRAIN_WINDOW_CIN = (2, 16, 32)          # lengths (csrc/train_window_moments.hip, csrc/train_window_flat.hip)
TRAIN_WINDOW_COUT = (16, 32, 64)
# geometries measured no faster than the composed path stay switched off here: none
TRAIN_WINDOW_OFF = frozenset()


def layer_train_window_ok(T: int, V: int, Ci: int, Co: int) -> bool:
    """Host arithmetic of `coskad_layer_train_window_ok`: a (Ci -> Co) layer of window length 8 / 16 / 24 trains on the stored-Z layer
    kernels (engine.chain_forward / chain_backward run it as they run a 12-frame layer).  False at T = 12.  Restated here so that
    building a train step needs no native library; tests/test_train_window_host.py holds the two in agreement."""
    return (T in WINDOW_LENGTHS and V in TRAIN_WINDOW_JOINTS and Ci in TRAIN_WINDOW_CIN and Co in TRAIN_WINDOW_COUT
            and (T, V) not in TRAIN_WINDOW_OFF)


# the few-channel set beside it: the virtual (4 -> 2) layer a stack's last (C -> 2) layer runs as by commutation.
# Geometries measured no faster than the autograd route of the decoder models stay switched off in a table of their own: none
TRAIN_WINDOW_NARROW = ((4, 2),)
TRAIN_WINDOW_NARROW_OFF = frozenset()


def layer_train_window_narrow_ok(T: int, V: int, Ci: int, Co: int) -> bool:
    """Host arithmetic of `coskad_layer_train_window_narrow_ok`: the few-channel (4 -> 2) layer of window length 8 / 16 / 24 trains on
    the stored-Z layer kernels.  A set of its own: `layer_train_window_ok` stays False there.  tests/test_ae_window_host.py holds the
    library and this restatement in agreement."""
    return (T in WINDOW_LENGTHS and V in TRAIN_WINDOW_JOINTS and (Ci, Co) in TRAIN_WINDOW_NARROW
            and (T, V) not in TRAIN_WINDOW_NARROW_OFF)


def gcn(x: Tensor, A: Tensor, Tm: Tensor, adjoint: bool = False) -> Tensor:
    """ConvTemporalGraphical.forward (reference stsgcn.py:143-156) or its adjoint."""
    N, C, T, V = x.shape
    _chk(x, "x"); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    out = torch.empty_like(x)
    call("coskad_gcn_f32", x, out, A, Tm, N * C, T, V, 1 if adjoint else 0, _stream())
    return out


def bn_fold(Wt, bt, gt, bet, mean_t, var_t, Wr, br, gr, ber, mean_r, var_r):
    """BN stats -> (wfold [2Ci, CoP], bias [CoP]) for layer_apply."""
    Co, Ci = Wt.shape[0], Wt.shape[1]
    for n, t in (("Wt", Wt), ("gamma_t", gt), ("beta_t", bet), ("mean_t", mean_t), ("var_t", var_t)):
        _chk(t, n)
    for n, t in (("bt", bt), ("Wr", Wr), ("br", br), ("gamma_r", gr), ("beta_r", ber), ("mean_r", mean_r), ("var_r", var_r)):
        _chk(t, n, optional=True)
    wfold = torch.empty(2 * Ci, cop(Co), device=Wt.device, dtype=torch.float32)
    bias = torch.empty(cop(Co), device=Wt.device, dtype=torch.float32)
    call("coskad_bn_fold_f32", Wt, bt, gt, bet, mean_t, var_t, Wr, br, gr, ber, mean_r, var_r, wfold, bias, Ci, Co, _stream())
    return wfold, bias


def layer_apply(x: Tensor, A: Tensor, Tm: Tensor, wfold: Tensor, bias: Tensor, Co: int,
                in_slope: Optional[Tensor] = None, out_slope: Optional[Tensor] = None,
                out: Optional[Tensor] = None) -> Tensor:
    """ST_GCNN_layer.forward with folded BN (reference stsgcn.py:94-116)."""
    B, Ci, T, V = x.shape
    _chk(x, "x"); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(bias, "bias", (cop(Co),))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(out_slope, "out_slope", (1,), optional=True)
    if out is None:
        out = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    else:
        _chk(out, "out", (B, Co, T, V))
    call("coskad_layer_apply_f32", x, out, A, Tm, wfold, bias, in_slope, out_slope, B, Ci, Co, T, V, _stream(), tag=(Ci, Co))
    return out


def layer_apply_window_ok(T: int, V: int, Ci: int, Co: int) -> bool:
    """layer_apply is ONE launch (folded BatchNorm, one clip per workgroup: csrc/eval_layer_clip.hip) at this window length other
    than 12; False at T = 12, whose layers `layer_fits` describes (the same kernel serves them at 17 / 25 joints)"""
    return bool(_lib.lib().coskad_layer_apply_window_ok(T, V, Ci, Co))


# (T, V) where the decoder-tail kernel measured no faster than the route without it stay switched off here
LAYER_TAIL_OFF = frozenset()


def layer_tail_ok(T: int, V: int, Ci: int, Co: int) -> bool:
    """layer_tail takes the (Ci -> Co) layer: 8 / 12 / 16 / 24 frames x 17 / 25 joints, 16 / 32 -> 2 channels (csrc/eval_tail_window.hip:
    `coskad_layer_tail_ok`) and the geometry is not switched off in LAYER_TAIL_OFF.  A set of its own: the other predicates stay False
    for two output channels."""
    return bool(_lib.lib().coskad_layer_tail_ok(T, V, Ci, Co)) and (T, V) not in LAYER_TAIL_OFF


def layer_tail(x_in: Tensor, A: Tensor, Tm: Tensor, wfold: Tensor, bias: Tensor, Co: int, in_slope: Optional[Tensor] = None,
               out_slope: Optional[Tensor] = None, x: Optional[Tensor] = None, want_out: bool = True, want_score: bool = False,
               out: Optional[Tensor] = None, score: Optional[Tensor] = None):
    """The last layer of an eval-mode decoder with folded BatchNorm (layer_apply's contract, two output channels) as one launch with
    one clip per workgroup, and -- `want_score`, against the target `x` [B, Co, T, V] -- the clip's mean squared reconstruction error
    from the same launch.  -> (out [B, Co, T, V] or None, score [B] or None); a clip's results do not depend on the batch."""
    B, Ci, T, V = x_in.shape
    _chk(x_in, "x_in"); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(bias, "bias", (cop(Co),))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(out_slope, "out_slope", (1,), optional=True)
    if not (want_out or want_score):
        raise ValueError("layer_tail: neither the reconstruction nor the score asked for")
    if want_score:
        _chk(x, "x", (B, Co, T, V))
        if score is None:
            score = torch.empty(B, device=x_in.device, dtype=torch.float32)
        else:
            _chk(score, "score", (B,))
    if want_out:
        if out is None:
            out = torch.empty(B, Co, T, V, device=x_in.device, dtype=torch.float32)
        else:
            _chk(out, "out", (B, Co, T, V))
    out, score = (out if want_out else None), (score if want_score else None)
    call("coskad_layer_tail_f32", x_in, x if want_score else None, out, score, A, Tm, wfold, bias, in_slope, out_slope, B, Ci, Co, T, V,
         _stream(), tag=(Ci, Co))
    return out, score


def layer_tail_map(x_in: Tensor, A: Tensor, Tm: Tensor, wfold: Tensor, bias: Tensor, Co: int, x: Tensor,
                   in_slope: Optional[Tensor] = None, out_slope: Optional[Tensor] = None, want_out: bool = False,
                   out: Optional[Tensor] = None, score: Optional[Tensor] = None, emap: Optional[Tensor] = None):
    """layer_tail's launch against the target `x` [B, Co, T, V] with the per-position map of the error beside the score:
    -> (out [B, Co, T, V] or None, score [B], emap [B, T, V] = ((out - x)^2).sum(1) / (Co T V)); emap[n].sum() is score[n], and score is
    bit for bit layer_tail's.  A clip's results do not depend on the batch."""
    B, Ci, T, V = x_in.shape
    _chk(x_in, "x_in"); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(bias, "bias", (cop(Co),))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(out_slope, "out_slope", (1,), optional=True)
    if not layer_tail_ok(T, V, Ci, Co):
        raise _lib.CoskadHipError(f"layer_tail_map: unsupported shape (n_frames={T}, n_joints={V}, C_in={Ci}, C_out={Co}): "
                                  "layer_tail_ok is False there, and nothing falls back")
    _chk(x, "x", (B, Co, T, V))
    if score is None:
        score = torch.empty(B, device=x_in.device, dtype=torch.float32)
    else:
        _chk(score, "score", (B,))
    if emap is None:
        emap = torch.empty(B, T, V, device=x_in.device, dtype=torch.float32)
    else:
        _chk(emap, "emap", (B, T, V))
    if want_out:
        if out is None:
            out = torch.empty(B, Co, T, V, device=x_in.device, dtype=torch.float32)
        else:
            _chk(out, "out", (B, Co, T, V))
    out = out if want_out else None
    call("coskad_layer_tail_map_f32", x_in, x, out, score, emap, A, Tm, wfold, bias, in_slope, out_slope, B, Ci, Co, T, V, _stream(),
         tag=(Ci, Co))
    return out, score, emap


INPUT_GRAD_FRAMES = (8, 12, 16, 24)     # window lengths, joint layouts, input and output widths of the folded layer's adjoint kernel
INPUT_GRAD_JOINTS = (17, 25)            # (csrc/eval_layer_adj.hip)
INPUT_GRAD_CIN = (2, 16, 32)
INPUT_GRAD_COUT = (16, 32, 64)


def layer_input_grad_ok(T: int, V: int, Ci: int, Co: int) -> bool:
    """Host arithmetic of `coskad_layer_input_grad_ok`: layer_input_grad takes the (Ci -> Co) layer at this geometry.  Restated here
    so that asking needs no native library; tests/test_attribution_host.py holds the two in agreement."""
    return T in INPUT_GRAD_FRAMES and V in INPUT_GRAD_JOINTS and Ci in INPUT_GRAD_CIN and Co in INPUT_GRAD_COUT


def layer_input_grad_max_grid(T: int, V: int, Ci: int, Co: int) -> int:
    """the persistent grid's cap (workgroups) of layer_input_grad at this shape; 0 where it is not built"""
    return int(_lib.lib().coskad_layer_input_grad_max_grid(T, V, Ci, Co))


def layer_input_grad(dU: Tensor, x_in: Tensor, A: Tensor, Tm: Tensor, wfold: Tensor, Co: int,
                     in_slope: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """The adjoint of layer_apply's folded layer with respect to its input `x_in` [B, Ci, T, V] (csrc/eval_layer_adj.hip):
    dIn [B, Ci, T, V] = PReLU'(x_in) (.) (gcn^T(Wz^T dU) + Wx^T dU) for dU [B, Co, T, V] and the `wfold` layer_apply takes.
    `in_slope` None (the network input): no mask, `x_in` gives the shape and is not read.
    One clip per workgroup: a clip's gradient does not depend on the batch it arrives in."""
    B, Co2, T, V = dU.shape
    if Co2 != Co:
        raise ValueError(f"layer_input_grad: dU has {Co2} channels, Co = {Co}")
    Ci = x_in.shape[1]
    _chk(dU, "dU"); _chk(x_in, "x_in", (B, Ci, T, V)); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(in_slope, "in_slope", (1,), optional=True)
    if out is None:
        out = torch.empty(B, Ci, T, V, device=dU.device, dtype=torch.float32)
    else:
        _chk(out, "out", (B, Ci, T, V))
    call("coskad_layer_input_grad_f32", dU, x_in if in_slope is not None else None, out, A, Tm, wfold, in_slope, B, Ci, Co, T, V,
         _stream(), tag=(Ci, Co))
    return out


def layer_first_pair_ok(Ci: int, Cm: int, Co: int, T: int, V: int) -> bool:
    """the first layer (2 -> Cm) and the layer behind it (Cm -> Co), folded, in one pass (csrc/eval_layer_clip.hip, FIRST form: 8 / 12 /
    16 / 24 frames)"""
    return bool(_lib.lib().coskad_layer_first_pair_ok(T, V, Ci, Cm, Co))


def layer_first_pair_apply(x: Tensor, A1: Tensor, T1: Tensor, wfold1: Tensor, bias1: Tensor, A2: Tensor, T2: Tensor, wfold2: Tensor,
                           bias2: Tensor, Cm: int, Co: int, mid_slope: Tensor, out_slope: Optional[Tensor] = None) -> Tensor:
    """layer_apply twice (folded BatchNorm: eval mode) for the first two layers of the encoder without the activation between them in
    HBM: x [B, 2, T, V] (the network input) -> [B, Co, T, V]; `mid_slope`: the first layer's PReLU weight."""
    B, Ci, T, V = x.shape
    _chk(x, "x", (B, 2, T, V)); _chk(A1, "A1", (T, V, V)); _chk(T1, "T1", (V, T, T)); _chk(A2, "A2", (T, V, V)); _chk(T2, "T2", (V, T, T))
    _chk(wfold1, "wfold1", (4, Cm)); _chk(bias1, "bias1", (Cm,)); _chk(wfold2, "wfold2", (2 * Cm, Co)); _chk(bias2, "bias2", (Co,))
    _chk(mid_slope, "mid_slope", (1,)); _chk(out_slope, "out_slope", (1,), optional=True)
    out = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    call("coskad_layer_first_pair_apply_f32", x, out, A1, T1, wfold1, bias1, A2, T2, wfold2, bias2, mid_slope, out_slope, B, Cm, Co, T, V,
         _stream())
    return out


def layer_fits(Ci: int, Co: int, T: int, V: int) -> bool:
    """Do the LDS-resident tile kernels take a (Ci -> Co) layer at this geometry?  (pure host arithmetic)"""
    return bool(_lib.lib().coskad_layer_fits(Ci, Co, T, V))


def stat_floats(Ci: int, Co: int) -> int:
    return _lib.lib().coskad_stat_floats(Ci, Co)


def train_stats_ws_bytes(Ci: int) -> int:
    return _lib.lib().coskad_train_stats_ws_bytes(Ci)


def layer_train_stats(x, A, Tm, in_slope, Wt, bt, gt, bet, rm_t, rv_t, nbt_t,
                      Wr, br, gr, ber, rm_r, rv_r, nbt_r, ws, momentum: float = 0.1, Z: Optional[Tensor] = None, ftabs=None):
    """Train-mode BN statistics of one layer -> (wfold, bias, stat); updates running stats in place.
    Z (optional, same shape as x): receives gcn(PReLU(x)) for layer_apply_z and the stored-Z backward.
    ftabs (optional; a stack's first layer, Z stored, T = 12, V = 17): build_ftabs' (As, Ts, tabs) -- the tables are built by extra
    blocks of the statistics pass's launch instead of a launch of their own."""
    B, Ci, T, V = x.shape
    Co = Wt.shape[0]
    _chk(x, "x"); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(Wt, "Wt", (Co, Ci)); _chk(gt, "gamma_t", (Co,)); _chk(bet, "beta_t", (Co,))
    for n, t in (("bt", bt), ("rm_t", rm_t), ("rv_t", rv_t), ("br", br), ("gamma_r", gr), ("beta_r", ber),
                 ("rm_r", rm_r), ("rv_r", rv_r)):
        _chk(t, n, (Co,), optional=True)
    _chk(Wr, "Wr", (Co, Ci), optional=True)
    _chk(in_slope, "in_slope", (1,), optional=True)
    _chk(nbt_t, "nbt_t", (), dtype=torch.int64, optional=True)
    _chk(nbt_r, "nbt_r", (), dtype=torch.int64, optional=True)
    need = train_stats_ws_bytes(Ci)
    if ws is None or ws.numel() * ws.element_size() < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    wfold = torch.empty(2 * Ci, cop(Co), device=x.device, dtype=torch.float32)
    bias = torch.empty(cop(Co), device=x.device, dtype=torch.float32)
    stat = torch.empty(stat_floats(Ci, Co), device=x.device, dtype=torch.float32)
    _chk(Z, "Z", tuple(x.shape), optional=True)
    args = (x, A, Tm, in_slope, Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r, nbt_r, momentum, wfold, bias, stat, ws,
            ws.numel() * ws.element_size(), B, Ci, Co, T, V, _stream())
    note_raw_write()
    if ftabs is not None:
        _chk(Z, "Z", tuple(x.shape))
        tab_A, tab_T, tabs, ntab = _ftab_pointers(*ftabs, T, V)
        call("coskad_layer_train_stats_z_ftab_f32", x, A, Tm, in_slope, Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r,
             nbt_r, momentum, wfold, bias, stat, ws, ws.numel() * ws.element_size(), B, Ci, Co, T, V, _stream(), Z, tab_A, tab_T, tabs,
             ntab)
    elif Z is None:
        call("coskad_layer_train_stats_f32", *args)
    else:
        call("coskad_layer_train_stats_z_f32", *args, Z)
    return wfold, bias, stat


# ---- SyncBN building blocks (csrc: "SyncBN" section of include/coskad_hip.h): batch reductions and folds as separate calls ---------
def layer_train_moments(x, A, Tm, in_slope, ws, Z: Optional[Tensor] = None) -> Tensor:
    """This rank's fp64 moment sums [sum xx^T Ci^2][sum x Ci][sum zz^T Ci^2][sum z Ci] of one layer's input (and Z = gcn(PReLU(x)))."""
    B, Ci, T, V = x.shape
    _chk(x, "x"); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T)); _chk(in_slope, "in_slope", (1,), optional=True)
    _chk(Z, "Z", tuple(x.shape), optional=True)
    need = train_stats_ws_bytes(Ci)
    if ws is None or _bytes(ws) < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    sums = torch.empty(2 * (Ci * Ci + Ci), device=x.device, dtype=torch.float64)
    call("coskad_layer_train_moments_f32", x, A, Tm, in_slope, Z, sums, ws, _bytes(ws), B, Ci, T, V, _stream())
    return sums


def layer_moment_sums(partials: Tensor, rows: int, Ci: int) -> Tensor:
    """fp64 sums of the moment partial rows a layer_apply_next wrote for the next layer."""
    _chk(partials, "partials")
    if partials.numel() < rows * 2 * (Ci * Ci + Ci):
        raise ValueError("layer_moment_sums: partials smaller than rows x 2 (Ci^2 + Ci)")
    sums = torch.empty(2 * (Ci * Ci + Ci), device=partials.device, dtype=torch.float64)
    call("coskad_layer_moment_sums_f32", partials, rows, Ci, sums, _stream())
    return sums


def layer_train_fold_sums(sums, count, Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r, nbt_r, momentum: float = 0.1):
    """(wfold, bias, stat) from moment sums over `count` positions (global clips x T x V once the ranks' sums are added)."""
    Co, Ci = Wt.shape
    _chk(sums, "sums", (2 * (Ci * Ci + Ci),), dtype=torch.float64); _chk(Wt, "Wt", (Co, Ci)); _chk(gt, "gamma_t", (Co,)); _chk(bet, "beta_t", (Co,))
    for n, t in (("bt", bt), ("rm_t", rm_t), ("rv_t", rv_t), ("br", br), ("gamma_r", gr), ("beta_r", ber), ("rm_r", rm_r), ("rv_r", rv_r)):
        _chk(t, n, (Co,), optional=True)
    _chk(Wr, "Wr", (Co, Ci), optional=True)
    _chk(nbt_t, "nbt_t", (), dtype=torch.int64, optional=True); _chk(nbt_r, "nbt_r", (), dtype=torch.int64, optional=True)
    wfold = torch.empty(2 * Ci, cop(Co), device=Wt.device, dtype=torch.float32)
    bias = torch.empty(cop(Co), device=Wt.device, dtype=torch.float32)
    stat = torch.empty(stat_floats(Ci, Co), device=Wt.device, dtype=torch.float32)
    note_raw_write()
    call("coskad_layer_train_fold_sums_f32", sums, float(count), Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r, nbt_r,
         momentum, wfold, bias, stat, Ci, Co, _stream())
    return wfold, bias, stat


def layer_bwd_stats(x_in, dU, A, Tm, in_slope, has_residual: bool, ws, Z=None):
    """Stage 1 of layer_bwd alone -> (chain buffer, rows): the partial rows, then their fp64 sums (chain_sums(buf, rows, Ci, Co))."""
    B, Ci, T, V = x_in.shape
    Co = dU.shape[1]
    _chk(x_in, "x_in"); _chk(dU, "dU", (B, Co, T, V)); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(Z, "Z", (B, Ci, T, V), optional=True)
    need = layer_bwd_ws_bytes(B, Ci, Co, T, V)
    if ws is None or _bytes(ws) < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    buf = torch.empty(_lib.lib().coskad_layer_bwd_stats_floats(B, Ci, Co, T, V), device=x_in.device, dtype=torch.float32)
    rows = ctypes.c_int(0)
    call("coskad_layer_bwd_stats_f32", x_in, dU, A, Tm, in_slope, 1 if has_residual else 0, buf, _bytes(buf), ctypes.byref(rows), ws,
         _bytes(ws), B, Ci, Co, T, V, _stream(), Z)
    return buf, rows.value


def chain_sums(buf: Tensor, rows: int, Ci: int, Co: int) -> Tensor:
    """The fp64 sums [P Co*Ci][Q Co*Ci][sdU Co] inside a backward chain buffer, as a view (all-reduce it in place for SyncBN)."""
    off = _lib.lib().coskad_layer_bwd_sums_offset(rows, Ci, Co)
    E = 2 * Co * Ci + Co
    return buf[off:off + 2 * E].view(torch.float64)


def layer_apply_z(Z, x, A, Tm, wfold, bias, Co, in_slope=None, out_slope=None, out=None):
    """U = Wz.Z + Wx.PReLU(x) + b from the stored Z = gcn(PReLU(x)) (training forward; streaming, no recompute)."""
    B, Ci, T, V = x.shape
    _chk(x, "x"); _chk(Z, "Z", (B, Ci, T, V)); _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(bias, "bias", (cop(Co),))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(out_slope, "out_slope", (1,), optional=True)
    if out is None:
        out = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    call("coskad_layer_apply_z_f32", Z, x, out, A, Tm, wfold, bias, in_slope, out_slope, B, Ci, Co, T, V, _stream())
    return out


def layer_apply_next_ok(Ci: int, Co: int, T: int, V: int) -> bool:
    """Does csrc/fused_apply_next.hip take a (Ci -> Co) layer (apply + the next layer's statistics in one kernel)?"""
    return bool(_lib.lib().coskad_layer_apply_next_ok(Ci, Co, T, V))


def layer_apply_next_rows(B: int, Ci: int, Co: int) -> int:
    """Partial rows layer_apply_next writes for a batch of B clips (each 2 (Co^2 + Co) floats)."""
    return _lib.lib().coskad_layer_apply_next_rows(B, Ci, Co)


def ftab_floats() -> int:
    return _lib.lib().coskad_ftab_floats()


def _ftab_pointers(As, Ts, tabs, T, V):
    """(A pointers, T pointers, table pointers, n) of up to 4 layers' forward mixing tables, checked"""
    n = len(As)
    if not (1 <= n <= 4) or len(Ts) != n or len(tabs) != n:
        raise ValueError("build_ftabs: 1..4 layers, equal list lengths")
    nf = ftab_floats()
    for A, Tm, tab in zip(As, Ts, tabs):
        _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T)); _chk(tab, "tab", (nf,))
    arr = ctypes.c_void_p * n
    return arr(*[t.data_ptr() for t in As]), arr(*[t.data_ptr() for t in Ts]), arr(*[t.data_ptr() for t in tabs]), n


def build_ftabs(As, Ts, tabs) -> None:
    """Forward mixing tables of up to 4 layers (lists of A [T,V,V], T [V,T,T], tab [ftab_floats()]) in one launch."""
    T, V = (As[0].shape[0], As[0].shape[1]) if len(As) else (0, 0)
    pa, pt, ptab, n = _ftab_pointers(As, Ts, tabs, T, V)
    call("coskad_build_ftab_f32", pa, pt, ptab, n, T, V, _stream())


def layer_apply_next(Z, x, wfold, bias, Co, in_slope, out_slope, ftab_next, partials, T, V, out=None, Z_next=None):
    """U = Wz.Z + Wx.PReLU(x) + b  AND  the next layer's Z_next = gcn_next(PReLU_out(U)) + its moment partials
    (csrc/fused_apply_next.hip).  -> (U, Z_next, rows): `rows` partial rows of 2 (Co^2 + Co) floats were written."""
    B, Ci = x.shape[0], x.shape[1]
    _chk(x, "x", (B, Ci, T, V)); _chk(Z, "Z", (B, Ci, T, V)); _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(bias, "bias", (cop(Co),))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(out_slope, "out_slope", (1,)); _chk(ftab_next, "ftab_next", (ftab_floats(),))
    _chk(partials, "partials")
    if out is None:
        out = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    if Z_next is None:
        Z_next = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    _chk(out, "out", (B, Co, T, V)); _chk(Z_next, "Z_next", (B, Co, T, V))
    rows = layer_apply_next_rows(B, Ci, Co)
    call("coskad_layer_apply_next_f32", Z, x, out, wfold, bias, in_slope, out_slope, ftab_next, Z_next, partials, _bytes(partials), B, Ci,
         Co, T, V, _stream(), tag=(Ci, Co))
    return out, Z_next, rows


def layer_apply_next_flat_ok(Ci: int, Co: int, T: int, V: int) -> bool:
    """apply + the next layer's statistics in one kernel on the 25-joint layout (csrc/fused_apply_flat.hip, NX form)"""
    return bool(_lib.lib().coskad_layer_apply_next_flat_ok(Ci, Co, T, V))


def layer_apply_next_flat(Z, x, wfold, bias, Co, in_slope, out_slope, A_next, T_next):
    """U = Wz.Z + Wx.PReLU(x) + b  AND  the next layer's Z_next = gcn_next(PReLU_out(U)) + its moment partials.
    -> (U, Z_next, partials, rows)"""
    B, Ci, T, V = x.shape
    _chk(x, "x"); _chk(Z, "Z", (B, Ci, T, V)); _chk(wfold, "wfold", (2 * Ci, cop(Co))); _chk(bias, "bias", (cop(Co),))
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(out_slope, "out_slope", (1,))
    _chk(A_next, "A_next", (T, V, V)); _chk(T_next, "T_next", (V, T, T))
    rows = int(_lib.lib().coskad_layer_apply_next_flat_rows(B))
    out = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    Zn = torch.empty(B, Co, T, V, device=x.device, dtype=torch.float32)
    partials = torch.empty(rows * 2 * (Co * Co + Co), device=x.device, dtype=torch.float32)
    call("coskad_layer_apply_next_flat_f32", Z, x, out, wfold, bias, in_slope, out_slope, A_next, T_next, Zn, partials, _bytes(partials), B,
         Ci, Co, T, V, _stream(), tag=(Ci, Co))
    return out, Zn, partials, rows


def layer_train_fold(partials, rows, B, T, V, Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r, nbt_r, ws,
                     momentum: float = 0.1):
    """The statistics of a layer from moment partials a previous layer_apply_next wrote -> (wfold, bias, stat)."""
    Co, Ci = Wt.shape
    _chk(partials, "partials"); _chk(Wt, "Wt", (Co, Ci)); _chk(gt, "gamma_t", (Co,)); _chk(bet, "beta_t", (Co,))
    for n, t in (("bt", bt), ("rm_t", rm_t), ("rv_t", rv_t), ("br", br), ("gamma_r", gr), ("beta_r", ber),
                 ("rm_r", rm_r), ("rv_r", rv_r)):
        _chk(t, n, (Co,), optional=True)
    _chk(Wr, "Wr", (Co, Ci), optional=True)
    _chk(nbt_t, "nbt_t", (), dtype=torch.int64, optional=True)
    _chk(nbt_r, "nbt_r", (), dtype=torch.int64, optional=True)
    if partials.numel() < rows * 2 * (Ci * Ci + Ci):
        raise ValueError("layer_train_fold: partials smaller than rows x 2 (Ci^2 + Ci)")
    need = train_stats_ws_bytes(Ci)
    if ws is None or _bytes(ws) < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    wfold = torch.empty(2 * Ci, cop(Co), device=Wt.device, dtype=torch.float32)
    bias = torch.empty(cop(Co), device=Wt.device, dtype=torch.float32)
    stat = torch.empty(stat_floats(Ci, Co), device=Wt.device, dtype=torch.float32)
    note_raw_write()
    call("coskad_layer_train_fold_f32", partials, rows, Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r, nbt_r, momentum,
         wfold, bias, stat, ws, _bytes(ws), B, Ci, Co, T, V, _stream())
    return wfold, bias, stat


def gather(src: Tensor, idx: Tensor) -> Tensor:
    """out[i] = src[idx[i]] (0 where idx < 0): operand streams of the fused encoder from the concatenated parameters."""
    _chk(src, "src"); _chk(idx, "idx", dtype=torch.int32)
    out = torch.empty(idx.shape, device=src.device, dtype=torch.float32)
    call("coskad_gather_f32", src, idx, out, idx.numel(), _stream())
    return out


def fused_encoder_out_floats() -> int:
    return _lib.lib().coskad_fused_encoder_out_floats()


def fused_encoder(x: Tensor, tab: Tensor, wreg: Tensor, slopes: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Eval-mode Encoder.forward (components.py:94-105) of the default stack in one kernel -> [B, KP]: the activated last
    layer in tile-major order (coskad_amd/fused_plan.py), zero in the padding columns."""
    B, C, T, V = x.shape
    _chk(x, "x"); _chk(tab, "tab"); _chk(wreg, "wreg"); _chk(slopes, "slopes", (4,))
    if C != 2:
        raise ValueError(f"fused_encoder: 2 input channels expected, got {C}")
    kp = fused_encoder_out_floats()
    if out is None:
        out = torch.empty(B, kp, device=x.device, dtype=torch.float32)
    else:
        _chk(out, "out", (B, kp))
    call("coskad_fused_encoder_f32", x, out, tab, wreg, slopes, B, T, V, _stream())
    return out


def layer_bwd_ws_bytes(B, Ci, Co, T, V) -> int:
    return _lib.lib().coskad_layer_bwd_ws_bytes(B, Ci, Co, T, V)


def layer_bwd_below_rows(B: int, Ci: int, Co: int, below_Ci: int, T: int, V: int) -> int:
    """Partial rows the (Ci -> Co) backward data kernel writes for the layer below it (0: that kernel cannot form them)."""
    return _lib.lib().coskad_layer_bwd_below_rows(B, Ci, Co, below_Ci, T, V)


def layer_bwd_below_floats(B: int, Ci: int, Co: int, below_Ci: int, T: int, V: int) -> int:
    """Floats of the chain buffer (partial rows + their fp64 sums) layer_bwd(..., below=...) fills for the layer below."""
    return _lib.lib().coskad_layer_bwd_below_floats(B, Ci, Co, below_Ci, T, V)


def layer_bwd(x_in, dU, A, Tm, in_slope, stat, Wt, gt, Wr, gr, grads: dict, ws, need_dx=True,
              dIn=None, accumulate=False, Z=None, stats_in=None, below=None, stats_count=0.0):
    """Backward of one layer.  `grads` maps names -> preallocated gradient tensors:
    A, T, Wt, bt (opt), gt, bet, Wr, br (opt), gr, ber, slope_in (opt).  Returns dIn (or None).
    Chain mode (csrc: coskad_layer_bwd_chain_f32, needs Z): `stats_in` = (partial rows tensor, rows) the call for the layer above
    wrote for this layer; `below` = (x_below, Z_below, in_slope_below, below_stats) makes this call write the layer below's partial rows;
    `stats_count`: positions the sums in `stats_in` cover (0: this batch; SyncBN: global clips x T x V)."""
    B, Ci, T, V = x_in.shape
    Co = Wt.shape[0]
    _chk(x_in, "x_in"); _chk(dU, "dU", (B, Co, T, V)); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(Wt, "Wt", (Co, Ci)); _chk(gt, "gamma_t", (Co,)); _chk(stat, "stat", (stat_floats(Ci, Co),))
    _chk(Wr, "Wr", (Co, Ci), optional=True); _chk(gr, "gamma_r", (Co,), optional=True)
    _chk(in_slope, "in_slope", (1,), optional=True)
    for k, shp in (("A", (T, V, V)), ("T", (V, T, T)), ("Wt", (Co, Ci)), ("gt", (Co,)), ("bet", (Co,))):
        _chk(grads[k], "grad " + k, shp)
    for k, shp in (("bt", (Co,)), ("Wr", (Co, Ci)), ("br", (Co,)), ("gr", (Co,)), ("ber", (Co,)), ("slope_in", (1,))):
        _chk(grads.get(k), "grad " + k, shp, optional=True)
    need = layer_bwd_ws_bytes(B, Ci, Co, T, V)
    if ws is None or _bytes(ws) < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    if need_dx and dIn is None:
        dIn = torch.empty_like(x_in)
    _chk(Z, "Z", (B, Ci, T, V), optional=True)
    args = (x_in, dU, A, Tm, in_slope, stat, Wt, gt, Wr, gr, dIn if need_dx else None, grads["A"], grads["T"], grads["Wt"],
            grads.get("bt"), grads["gt"], grads["bet"], grads.get("Wr"), grads.get("br"), grads.get("gr"), grads.get("ber"),
            grads.get("slope_in"), ws, _bytes(ws), 1 if accumulate else 0, B, Ci, Co, T, V, _stream())
    if stats_in is not None or below is not None:
        if Z is None:
            raise ValueError("layer_bwd: chain mode needs the stored Z")
        sp, srows = stats_in if stats_in is not None else (None, 0)
        _chk(sp, "stats_in", optional=True)
        if sp is not None and sp.numel() < (srows * (2 * Co * Ci + Co) + 1) // 2 * 2 + 2 * (2 * Co * Ci + Co):
            raise ValueError("layer_bwd: stats_in smaller than a chain buffer of that many rows")
        xb, zb, sb, bs = below if below is not None else (None, None, None, None)
        cb = xb.shape[1] if xb is not None else 0
        _chk(xb, "below x", (B, cb, T, V), optional=True); _chk(zb, "below Z", (B, cb, T, V), optional=True); _chk(bs, "below_stats", optional=True)
        _chk(sb, "below in_slope", (1,), optional=True)
        call("coskad_layer_bwd_chain_f32", *args, Z, sp, srows, _bytes(sp) if sp is not None else 0, xb, zb, sb, cb, bs,
             _bytes(bs) if bs is not None else 0, float(stats_count))
    elif Z is None:
        call("coskad_layer_bwd_f32", *args)
    else:       # stored gcn(PReLU(x_in)) from layer_train_stats(..., Z=...): no mixing recompute in the backward kernels
        call("coskad_layer_bwd_z_f32", *args, Z)
    return dIn if need_dx else None


def layer_bwd_data(x_in, dU, A, Tm, in_slope, stat, Wt, gt, Wr, gr, grads: dict, ws, dZ, need_dx=True, dIn=None,
                   accumulate=False, Z=None):
    """Stages 1-3 of layer_bwd (everything but dA, dT); dZ [B,Ci,T,V] receives the mixing-output gradient that
    layer_gcn_params consumes (possibly on another stream).  Returns dIn (or None)."""
    B, Ci, T, V = x_in.shape
    Co = Wt.shape[0]
    _chk(x_in, "x_in"); _chk(dU, "dU", (B, Co, T, V)); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(Wt, "Wt", (Co, Ci)); _chk(gt, "gamma_t", (Co,)); _chk(stat, "stat", (stat_floats(Ci, Co),))
    _chk(Wr, "Wr", (Co, Ci), optional=True); _chk(gr, "gamma_r", (Co,), optional=True)
    _chk(in_slope, "in_slope", (1,), optional=True); _chk(dZ, "dZ", (B, Ci, T, V)); _chk(Z, "Z", (B, Ci, T, V), optional=True)
    for k, shp in (("Wt", (Co, Ci)), ("gt", (Co,)), ("bet", (Co,))):
        _chk(grads[k], "grad " + k, shp)
    for k, shp in (("bt", (Co,)), ("Wr", (Co, Ci)), ("br", (Co,)), ("gr", (Co,)), ("ber", (Co,)), ("slope_in", (1,))):
        _chk(grads.get(k), "grad " + k, shp, optional=True)
    need = layer_bwd_ws_bytes(B, Ci, Co, T, V)
    if ws is None or _bytes(ws) < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    if need_dx and dIn is None:
        dIn = torch.empty_like(x_in)
    call("coskad_layer_bwd_data_f32", x_in, dU, A, Tm, in_slope, stat, Wt, gt, Wr, gr, dIn if need_dx else None, dZ, grads["Wt"],
         grads.get("bt"), grads["gt"], grads["bet"], grads.get("Wr"), grads.get("br"), grads.get("gr"), grads.get("ber"),
         grads.get("slope_in"), ws, _bytes(ws), 1 if accumulate else 0, B, Ci, Co, T, V, _stream(), Z)
    return dIn if need_dx else None


def layer_gcn_params_ws_bytes(T, V) -> int:
    return _lib.lib().coskad_layer_gcn_params_ws_bytes(T, V)


def layer_gcn_params(x_in, in_slope, dZ, A, Tm, dA, dT, ws, accumulate=False):
    """dA, dT of one layer from its stored input and dZ (enqueued on the CURRENT torch stream)."""
    B, Ci, T, V = x_in.shape
    _chk(x_in, "x_in"); _chk(dZ, "dZ", (B, Ci, T, V)); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    _chk(dA, "dA", (T, V, V)); _chk(dT, "dT", (V, T, T)); _chk(in_slope, "in_slope", (1,), optional=True)
    if ws is None or _bytes(ws) < layer_gcn_params_ws_bytes(T, V):
        raise ValueError("workspace too small")
    call("coskad_layer_gcn_params_f32", x_in, in_slope, dZ, A, Tm, dA, dT, ws, _bytes(ws), 1 if accumulate else 0, B, Ci, T, V, _stream())


def btlnk_fwd(U: Tensor, W: Tensor, bias: Optional[Tensor], slope: Optional[Tensor], ws=None) -> Tensor:
    """z = Linear(flatten(PReLU(U)))  (reference ae.py:97-101).  ws: an engine.Workspace to take the split-K scratch from
    (stream-ordered reuse across the kernels of one module); None allocates it per call."""
    B = U.shape[0]
    K = U.numel() // B
    L = W.shape[0]
    _chk(U, "U"); _chk(W, "W", (L, K)); _chk(bias, "bias", (L,), optional=True); _chk(slope, "slope", (1,), optional=True)
    z = torch.empty(B, L, device=U.device, dtype=torch.float32)
    if L > 16:
        # 16 < L <= 512: the LDS-tiled MFMA GEMM of csrc/btlnk_wide.hip, K slices summed in a fixed order (any K)
        nbytes = _lib.lib().coskad_btlnk_fwd_ws_bytes_l(B, K, L)
        buf = ws.get(nbytes, U.device) if ws is not None else torch.empty(nbytes, dtype=torch.uint8, device=U.device)
        call("coskad_btlnk_fwd_ws_f32", U, W, bias, slope, z, buf, nbytes, B, K, L, _stream())
        return z
    if B >= BTLNK_SPLITK_MIN_B and K % 16 == 0:
        # blocks of 64 clips x 4 K slices (W operands shared by four clip tiles), fixed-order partial sums
        nbytes = _lib.lib().coskad_btlnk_fwd_ws_bytes(B)
        buf = ws.get(nbytes, U.device) if ws is not None else torch.empty(nbytes, dtype=torch.uint8, device=U.device)
        call("coskad_btlnk_fwd_ws_f32", U, W, bias, slope, z, buf, nbytes, B, K, L, _stream())
        return z
    call("coskad_btlnk_fwd_f32", U, W, bias, slope, z, B, K, L, _stream())
    return z


BTLNK_SPLITK_MIN_B = 1      # always (K % 16 == 0): a clip's latent must not depend on the batch it arrives in (bit-exact chunking)
BTLNK_LMAX = 512            # widest latent of the bottleneck and head kernels (csrc/btlnk_wide.hip, csrc/heads.hip)


def btlnk_bwd_ws_bytes(B, K, L) -> int:
    return _lib.lib().coskad_btlnk_bwd_ws_bytes(B, K, L)


def btlnk_bwd(U, W, dz, slope, dW, db, dslope, ws, dU=None, accumulate=False):
    B = U.shape[0]
    K = U.numel() // B
    L = W.shape[0]
    _chk(U, "U"); _chk(W, "W", (L, K)); _chk(dz, "dz", (B, L)); _chk(dW, "dW", (L, K))
    _chk(db, "db", (L,), optional=True); _chk(dslope, "dslope", (1,), optional=True); _chk(slope, "slope", (1,), optional=True)
    need = btlnk_bwd_ws_bytes(B, K, L)
    if ws is None or _bytes(ws) < need:
        raise ValueError(f"workspace too small: need {need} bytes")
    if dU is None:
        dU = torch.empty_like(U)
    call("coskad_btlnk_bwd_f32", U, W, dz, slope, dU, dW, db, dslope, ws, _bytes(ws), 1 if accumulate else 0, B, K, L, _stream())
    return dU


def btlnk_bwd_chain_ok(K: int, TV: int, below_Ci: int) -> bool:
    """coskad_btlnk_bwd_chain_f32 takes the shape: a 64-channel last layer over 16 / 32 input channels."""
    return bool(_lib.lib().coskad_btlnk_bwd_chain_ok(K, TV, below_Ci))


def btlnk_bwd_chain(U, W, dz, slope, dW, db, dslope, ws, below_in, below_Z, below_in_slope, dU=None, accumulate=False):
    """btlnk_bwd AND the top layer's backward batch reductions from one pass (csrc/btlnk_chain.hip).
    U [B, 64, T, V]: the top layer's pre-activation; below_in / below_Z [B, Ci, T, V]: that layer's input (pre-activation of the
    layer below + its slope) and stored gcn output.  -> (dU, (chain buffer, rows)): the second item is layer_bwd's `stats_in`.
    `ws`: an engine.Workspace."""
    B, Ch, T, V = U.shape
    TV = T * V
    K = Ch * TV
    L = W.shape[0]
    Ci = below_in.shape[1]
    _chk(U, "U"); _chk(W, "W", (L, K)); _chk(dz, "dz", (B, L)); _chk(dW, "dW", (L, K))
    _chk(db, "db", (L,), optional=True); _chk(dslope, "dslope", (1,), optional=True); _chk(slope, "slope", (1,), optional=True)
    _chk(below_in, "below_in", (B, Ci, T, V)); _chk(below_Z, "below_Z", (B, Ci, T, V)); _chk(below_in_slope, "below_in_slope", (1,), optional=True)
    if not btlnk_bwd_chain_ok(K, TV, Ci):
        raise ValueError(f"btlnk_bwd_chain: shape K={K} TV={TV} Ci={Ci} not supported")
    lib = _lib.lib()
    need = lib.coskad_btlnk_bwd_chain_ws_bytes(B, K, L, TV)
    buf = ws.get(need, U.device)
    stats = torch.empty(lib.coskad_btlnk_bwd_chain_floats(B, TV, Ci), device=U.device, dtype=torch.float32)
    if dU is None:
        dU = torch.empty_like(U)
    rows = ctypes.c_int(0)
    call("coskad_btlnk_bwd_chain_f32", U, W, dz, slope, dU, dW, db, dslope, buf, _bytes(buf), 1 if accumulate else 0, B, K, L, below_in,
         below_Z, below_in_slope, Ci, TV, stats, _bytes(stats), ctypes.byref(rows), _stream())
    return dU, (stats, rows.value)


def btlnk_fwd_parts(U: Tensor, W: Tensor, slope: Optional[Tensor]) -> Tensor:
    """The split-K partials [KS, B, 16] of btlnk_fwd's large-batch path without the launch that sums them (L <= 16, K % 16 == 0):
    z = part.sum(0)[:, :L] + bias, in slice order, is left to btlnk_bwd_chain_head."""
    B = U.shape[0]
    K = U.numel() // B
    L = W.shape[0]
    _chk(U, "U"); _chk(W, "W", (L, K)); _chk(slope, "slope", (1,), optional=True)
    part = torch.empty(_lib.lib().coskad_btlnk_fwd_ks(), B, 16, device=U.device, dtype=torch.float32)
    call("coskad_btlnk_fwd_parts_f32", U, W, slope, part, _bytes(part), B, K, L, _stream())
    return part


def btlnk_bwd_chain_head(U, W, part, bias, c, slope, dW, db, dslope, ws, below_in, below_Z, below_in_slope, acc=None, need_score=False,
                         upstream=1.0, dU=None, accumulate=False):
    """btlnk_fwd's summing launch, mse_head and btlnk_bwd_chain in the launches of the last (csrc/btlnk_chain.hip, HD form): from the
    partials of btlnk_fwd_parts, the Linear's bias and the centre c -> (z, dz, score or None, stats, dU, (chain buffer, rows)), every
    value bit-identical to the three calls; acc (+)= the head's raw sums.  `ws`: an engine.Workspace."""
    B, Ch, T, V = U.shape
    TV = T * V
    K = Ch * TV
    L = W.shape[0]
    Ci = below_in.shape[1]
    KS = part.shape[0]
    S = head_slots(L)
    _chk(U, "U"); _chk(W, "W", (L, K)); _chk(part, "part", (KS, B, 16)); _chk(bias, "bias", (L,), optional=True); _chk(c, "c", (L,))
    _chk(dW, "dW", (L, K)); _chk(db, "db", (L,), optional=True); _chk(dslope, "dslope", (1,), optional=True)
    _chk(slope, "slope", (1,), optional=True); _chk(acc, "acc", (S,), optional=True)
    _chk(below_in, "below_in", (B, Ci, T, V)); _chk(below_Z, "below_Z", (B, Ci, T, V)); _chk(below_in_slope, "below_in_slope", (1,), optional=True)
    if not btlnk_bwd_chain_ok(K, TV, Ci):
        raise ValueError(f"btlnk_bwd_chain_head: shape K={K} TV={TV} Ci={Ci} not supported")
    lib = _lib.lib()
    need = lib.coskad_btlnk_bwd_chain_ws_bytes(B, K, L, TV)
    buf = ws.get(need, U.device)
    chain = torch.empty(lib.coskad_btlnk_bwd_chain_floats(B, TV, Ci), device=U.device, dtype=torch.float32)
    if dU is None:
        dU = torch.empty_like(U)
    z = torch.empty(B, L, device=U.device, dtype=torch.float32)
    dz = torch.empty_like(z)
    score = torch.empty(B, device=U.device, dtype=torch.float32) if need_score else None
    stats = torch.empty(S, device=U.device, dtype=torch.float32)
    hws = head_ws(B, U.device, L)
    rows = ctypes.c_int(0)
    call("coskad_btlnk_bwd_chain_head_f32", U, W, part, KS, bias, c, upstream, z, dz, score, stats, acc, hws, slope, dU, dW, db, dslope,
         buf, _bytes(buf), 1 if accumulate else 0, B, K, L, below_in, below_Z, below_in_slope, Ci, TV, chain, _bytes(chain),
         ctypes.byref(rows), _stream())
    return z, dz, score, stats, dU, (chain, rows.value)


def _cuda_f32(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise _lib.CoskadHipError(f"{name}: expected a CUDA (ROCm) tensor, got device {t.device}; no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")


def _b3(t: Tensor):
    """(tensor viewed as [batch, rows, cols], element strides) -- 2-D operands broadcast over the batch (stride 0)."""
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1], 0, t.stride(0), t.stride(1)
    if t.dim() == 3:
        return t.shape[0], t.shape[1], t.shape[2], t.stride(0), t.stride(1), t.stride(2)
    raise ValueError("gemm operands are 2-D or 3-D")


def gemm(A: Tensor, B: Tensor, out: Optional[Tensor] = None, bias: Optional[Tensor] = None, bias_mode: int = 0,
         bias_mod: int = 1, relu: bool = False, accumulate: bool = False) -> Tensor:
    """C[b] = act(A[b] @ B[b] + bias) on the fp32 MFMA GEMM kernel; A [.., M, K], B [.., K, N] may be ANY strided views
    (transposes, broadcast batch): nothing is copied."""
    _cuda_f32(A, "A"); _cuda_f32(B, "B")
    ba, M, K, sab, sam, sak = _b3(A)
    bb, K2, N, sbb, sbk, sbn = _b3(B)
    if K != K2:
        raise ValueError(f"gemm: inner sizes differ ({K} vs {K2})")
    batch = max(ba, bb)
    if ba not in (1, batch) or bb not in (1, batch):
        raise ValueError("gemm: batch sizes do not broadcast")
    if ba == 1:
        sab = 0
    if bb == 1:
        sbb = 0
    if out is None:
        out = torch.empty((batch, M, N) if (A.dim() == 3 or B.dim() == 3) else (M, N), device=A.device, dtype=torch.float32)
    _cuda_f32(out, "out")
    bc, Mc, Nc, scb, scm, scn = _b3(out)
    if (Mc, Nc) != (M, N) or bc != batch:
        raise ValueError(f"gemm: out has shape {tuple(out.shape)}, expected batch {batch} x {M} x {N}")
    _chk(bias, "bias", optional=True)
    call("coskad_gemm_f32", A, B, out, bias, sab, sam, sak, sbb, sbk, sbn, scb, scm, scn, M, N, K, batch, bias_mode, bias_mod,
         1 if relu else 0, 0, 0, 0, 1 if accumulate else 0, _stream())
    return out


def gemm_reduce(A: Tensor, B: Tensor, out: Tensor, target_chunks: int = 64, ktotal: int = 0, accumulate: bool = False) -> Tensor:
    """out (+)= sum_b A[b] @ B[b] (weight gradients): partial sums per batch chunk on the GEMM kernel, then a fixed-order
    fp64 sum.  ktotal > 0: the reduction axis is one long axis cut into `batch` pieces of K (the last one partial)."""
    _cuda_f32(A, "A"); _cuda_f32(B, "B"); _chk(out, "out")
    ba, M, K, sab, sam, sak = _b3(A)
    bb, K2, N, sbb, sbk, sbn = _b3(B)
    if K != K2 or ba != bb or tuple(out.shape) != (M, N):
        raise ValueError("gemm_reduce: shape mismatch")
    chunk = max(1, (ba + target_chunks - 1) // target_chunks)
    chunks = (ba + chunk - 1) // chunk
    part = torch.empty(chunks, M, N, device=A.device, dtype=torch.float32)
    call("coskad_gemm_f32", A, B, part, None, sab, sam, sak, sbb, sbk, sbn, 0, 0, 0, M, N, K, ba, 0, 1, 0, 1, chunk, ktotal, 0, _stream())
    call("coskad_gemm_sum_f32", part, chunks, M * N, out, 1 if accumulate else 0, _stream())
    return out


def gemm_rows_outer(G: Tensor, S: Tensor, out: Tensor, rows_per_piece: int = 256, target_chunks: int = 64,
                    accumulate: bool = False) -> Tensor:
    """out[m, n] (+)= sum_r G[r, m] * S[r, n] for row-major G [R, M], S [R, N]: the long reduction axis r is cut into pieces
    of `rows_per_piece` (the kernel's batch axis, the last piece guarded by ktotal = R), pieces are summed per chunk."""
    R, M = G.shape
    R2, N = S.shape
    _chk(G, "G"); _chk(S, "S"); _chk(out, "out", (M, N))
    if R != R2:
        raise ValueError("gemm_rows_outer: row counts differ")
    nb = (R + rows_per_piece - 1) // rows_per_piece
    chunk = max(1, (nb + target_chunks - 1) // target_chunks)
    chunks = (nb + chunk - 1) // chunk
    part = torch.empty(chunks, M, N, device=G.device, dtype=torch.float32)
    call("coskad_gemm_f32", G, S, part, None, rows_per_piece * M, 1, M, rows_per_piece * N, N, 1, 0, 0, 0, M, N, rows_per_piece, nb, 0, 1,
         0, 1, chunk, R, 0, _stream())
    call("coskad_gemm_sum_f32", part, chunks, M * N, out, 1 if accumulate else 0, _stream())
    return out


def conv1x1_ok(M: int, K: int, P: int) -> bool:
    return bool(_lib.lib().coskad_conv1x1_ok(M, K, P))


def conv1x1(W: Tensor, x: Tensor, bias: Optional[Tensor] = None, out: Optional[Tensor] = None, accumulate: bool = False,
            want_stats: bool = False):
    """out[b] (+)= W @ x[b] (+ bias) for W [M, K] (any 2-D view contiguous along one axis: pass `w.t()` for the data gradient),
    x [B, K, P] contiguous -> (out [B, M, P], stats partials or None).  Shapes outside csrc/conv1x1.hip go to the strided GEMM."""
    M, K = W.shape
    B, K2, P = x.shape
    _cuda_f32(W, "W"); _chk(x, "x"); _chk(bias, "bias", (M,), optional=True)
    if K != K2:
        raise ValueError(f"conv1x1: weight has {K} input channels, x has {K2}")
    sm, sk = W.stride(0), W.stride(1)
    fast = conv1x1_ok(M, K, P) and (sk == 1 or sm == 1) and (sm % 4 == 0 if sk == 1 else sk % 4 == 0) and W.data_ptr() % 16 == 0 \
        and x.data_ptr() % 16 == 0
    if out is None:
        out = torch.empty(B, M, P, device=x.device, dtype=torch.float32)
    _chk(out, "out", (B, M, P))
    if not fast or out.data_ptr() % 16 != 0:
        gemm(W, x, out=out, bias=bias, bias_mode=1 if bias is not None else 0, bias_mod=M, accumulate=accumulate)
        return out, None
    parts = None
    if want_stats:
        rows = _lib.lib().coskad_conv1x1_stat_rows(M, K, P, B)
        parts = torch.empty(rows, M, 2, device=x.device, dtype=torch.float64)
    call("coskad_conv1x1_f32", W, sm, sk, x, out, bias, parts, M, K, P, B, 1 if accumulate else 0, _stream())
    return out, parts


WGRAD_BLOCKS = 256   # workgroups a weight-gradient launch aims for (one per CU; sweep 64..2048: wide step 19.7 / 18.0 / 18.2 / 18.7 / 19.5 ms at 64 / 256 / 512 / 1024 / 2048)


def conv1x1_wgrad(G: Tensor, x: Tensor, out: Tensor, target_chunks: int = 64, accumulate: bool = False) -> Tensor:
    """out[m, k] (+)= sum_b sum_p G[b, m, p] x[b, k, p]: the weight gradient of a 1x1 convolution (G [B, M, P], x [B, K, P]).
    csrc/conv1x1.hip where the shape allows, the strided GEMM's chunked reduction otherwise; deterministic either way."""
    B, M, P = G.shape
    K = x.shape[1]
    _chk(G, "G"); _chk(x, "x", (B, K, P)); _chk(out, "out", (M, K))
    if not _lib.lib().coskad_conv1x1_wgrad_ok(M, K, P) or G.data_ptr() % 16 or x.data_ptr() % 16:
        return gemm_reduce(G, x.transpose(1, 2), out, target_chunks=target_chunks, accumulate=accumulate)
    # the kernel's grid is (K tiles, M tiles, clip chunks): enough chunks for ~WGRAD_BLOCKS workgroups (narrow layers have ONE tile)
    tm, tk = (128, 128) if (M % 128 == 0 and K % 128 == 0) else ((64, 64) if M % 64 == 0 else (32, 64))
    tiles = (M // tm) * (K // tk)
    target_chunks = max(target_chunks, -(-WGRAD_BLOCKS // tiles))
    chunk = max(1, (B + target_chunks - 1) // target_chunks)
    chunks = (B + chunk - 1) // chunk
    part = torch.empty(chunks, M, K, device=G.device, dtype=torch.float32)
    call("coskad_conv1x1_wgrad_f32", G, x, part, M, K, P, B, chunk, _stream())
    call("coskad_gemm_sum_f32", part, chunks, M * K, out, 1 if accumulate else 0, _stream())
    return out


def bn_momentum(bn) -> float:
    """nn.BatchNorm's `exponential_average_factor` for ONE training-mode forward (torch/nn/modules/batchnorm.py, _BatchNorm.forward):
    the fixed `momentum`, or with momentum=None the cumulative moving average 1 / num_batches_tracked, counted after this batch.  The
    kernels increment the device counter through its raw pointer; the host keeps a mirror of it so that no forward waits for the
    device -- re-read (one .item()) whenever torch itself wrote the tensor (load_state_dict, fill_: its version counter moves).
    Call exactly once per BatchNorm and training forward."""
    if bn.momentum is not None:
        return float(bn.momentum)
    nbt = bn.num_batches_tracked
    if nbt is None:                       # track_running_stats=False: nothing to average
        return 0.0
    st = bn.__dict__.get("_coskad_nbt")
    n = st[2] if (st is not None and st[0] is nbt and st[1] == nbt._version) else int(nbt.item())
    bn.__dict__["_coskad_nbt"] = (nbt, nbt._version, n + 1)
    return 1.0 / (n + 1)


def bn_batch_stats(bn, training: bool) -> bool:
    """does this BatchNorm normalise with batch statistics in this mode? (track_running_stats=False: always, batchnorm.py's `bn_training`)"""
    return bool(training) or bn.running_mean is None or bn.running_var is None


def bn2_stats_parts(parts: Tensor, bn, count: int) -> Tensor:
    """Train-mode statistics of nn.BatchNorm2d `bn` from the partial sums a conv1x1 epilogue wrote (+ running update)."""
    rows, C, _ = parts.shape
    _chk(parts, "parts", (rows, C, 2), dtype=torch.float64)
    stat = torch.empty(2 * C, device=parts.device, dtype=torch.float32)
    note_raw_write()
    call("coskad_bn2_stats_parts_f32", parts, rows, stat, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn_momentum(bn), bn.eps,
         float(count), C, _stream())
    return stat


def relu_bwd(out: Tensor, dout: Tensor, dbias: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """g = dout * (out > 0) on [N, C, P]; dbias[c] (+)= sum of g over (n, p)."""
    Nb, C, P = out.shape
    _chk(out, "out"); _chk(dout, "dout", (Nb, C, P)); _chk(dbias, "dbias", (C,), optional=True)
    g = torch.empty_like(out)
    slices = min(Nb, 64)
    part = torch.empty(slices, C, device=out.device, dtype=torch.float32)
    call("coskad_relu_bwd_f32", out, dout, g, part, Nb, C, P, slices, _stream())
    if dbias is not None:
        call("coskad_gemm_sum_f32", part, slices, C, dbias, 1 if accumulate else 0, _stream())
    return g


def softmax_rows(x: Tensor) -> Tensor:
    n = x.shape[0]
    _chk(x, "x", (n, n))
    y = torch.empty_like(x)
    call("coskad_softmax_rows_f32", x, y, n, _stream())
    return y


def softmax_rows_bwd(y: Tensor, dy: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out: where dx goes (a flat gradient view), a fresh tensor otherwise"""
    n = y.shape[0]
    _chk(y, "y", (n, n)); _chk(dy, "dy", (n, n)); _chk(out, "out", (n, n), optional=True)
    dx = torch.empty_like(y) if out is None else out
    call("coskad_softmax_rows_bwd_f32", y, dy, dx, n, _stream())
    return dx


PLAIN_GCN_CMAX = 64                               # widest channel count of the fused plain-GCN kernels (csrc/plain_gcn.hip)
PLAIN_GCN_POSITIONS = (168, 204, 216, 300)        # 12 frames x JOINT_LAYOUTS


def plain_gcn_ok(Ci: int, Co: int, P: int) -> bool:
    """Host arithmetic of `coskad_plain_gcn_ok`: the fused plain-GCN kernels take a (Ci -> Co) layer on P = T * V positions; other
    shapes are composed from the strided GEMM.  Restated here so that building a model needs no native library;
    tests/test_plain_gcn_host.py holds the two in agreement."""
    return 1 <= Ci <= PLAIN_GCN_CMAX and 1 <= Co <= PLAIN_GCN_CMAX and P in PLAIN_GCN_POSITIONS


def plain_gcn_fwd(X: Tensor, W: Tensor, Ap: Tensor, bias: Optional[Tensor] = None, save: bool = False, grid_cap: int = 0):
    """O[b] = relu(W^T . X[b] . A'^T + bias) in one launch (csrc/plain_gcn.hip): X [B, Ci, P], W [Ci, Co], A' [P, P] -> (O [B, Co, P],
    S).  save: S is the narrow-side intermediate (Y = X . A'^T [B, Ci, P] when Ci <= Co, H = W^T . X [B, Co, P] otherwise) for the
    backward; None otherwise -- it then never leaves the chip."""
    B, Ci, P = X.shape
    Co = W.shape[1]
    _chk(X, "X"); _chk(W, "W", (Ci, Co)); _chk(Ap, "Ap", (P, P)); _chk(bias, "bias", (Co,), optional=True)
    O = torch.empty(B, Co, P, device=X.device, dtype=torch.float32)
    S = torch.empty(B, min(Ci, Co), P, device=X.device, dtype=torch.float32) if save else None
    call("coskad_plain_gcn_fwd_f32", X, W, Ap, bias, O, S, B, Ci, Co, P, grid_cap, _stream(), tag=(Ci, Co))
    return O, S


def plain_gcn_bwd(X: Tensor, S: Optional[Tensor], O: Tensor, dO: Tensor, W: Tensor, Ap: Tensor, dW: Tensor, db: Optional[Tensor],
                  need_dx: bool = True, need_da: bool = False, accumulate: bool = False, grid_cap: int = 0):
    """Backward of plain_gcn_fwd in one launch + the fixed-order reduction of its partial rows: dW [Ci, Co] and db [Co] (None: no
    bias) are written (accumulate: added to) in place -> (dX [B, Ci, P] or None, D or None).  S: plain_gcn_fwd's saved intermediate
    (needed when Ci <= Co).  need_da: D is the narrow-side gradient for the adjacency gradient
    dA'[q, p] = sum_rows D[r, q] Src[r, p], Src = X (Ci <= Co) or the saved H (Ci > Co) -- ops.gemm_rows_outer."""
    B, Ci, P = X.shape
    Co = W.shape[1]
    Cn = min(Ci, Co)
    _chk(X, "X"); _chk(W, "W", (Ci, Co)); _chk(Ap, "Ap", (P, P)); _chk(O, "O", (B, Co, P)); _chk(dO, "dO", (B, Co, P))
    _chk(S, "S", (B, Cn, P), optional=Ci > Co); _chk(dW, "dW", (Ci, Co)); _chk(db, "db", (Co,), optional=True)
    nws = _lib.lib().coskad_plain_gcn_ws_bytes(B, Ci, Co, P, grid_cap)
    ws = torch.empty(max(nws, 4), dtype=torch.uint8, device=X.device)
    dX = torch.empty_like(X) if need_dx else None
    D = torch.empty(B, Cn, P, device=X.device, dtype=torch.float32) if need_da else None
    call("coskad_plain_gcn_bwd_f32", X, S, O, dO, W, Ap, dX, dW, db, D, ws, nws, B, Ci, Co, P, 1 if need_dx else 0, 1 if need_da else 0,
         1 if accumulate else 0, grid_cap, _stream(), tag=(Ci, Co))
    return dX, D


def _bn2_ws(Nb: int, C: int, device, bwd: bool = False) -> Tensor:
    lib = _lib.lib()
    nbytes = lib.coskad_bn2_bwd_ws_bytes(Nb, C) if bwd else lib.coskad_bn2_ws_bytes(Nb, C)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def bn2_stats(x: Tensor, bn, training: bool) -> Tensor:
    """Per-channel (mean, invstd) of x [N, C, P] for nn.BatchNorm2d `bn`: batch statistics (+ running update) in training
    mode, the running statistics otherwise."""
    Nb, C, P = x.shape
    _chk(x, "x")
    stat = torch.empty(2 * C, device=x.device, dtype=torch.float32)
    ws = _bn2_ws(Nb, C, x.device)
    if training:
        note_raw_write()
    call("coskad_bn2_stats_f32", x, stat, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn_momentum(bn) if training else 0.0,
         bn.eps, 1 if training else 0, ws, ws.numel(), Nb, C, P, _stream())
    return stat


def bn2_apply_prelu(Ct, Cr, stat_t, gt, bt, stat_r, gr, br, slope, drop_p: float = 0.0, drop_seed: int = 0) -> Tensor:
    """out = PReLU(Dropout_p(BN_t(Ct)) + BN_r(Cr)); the dropout mask is a counter-based function of (drop_seed, element)."""
    Nb, C, P = Ct.shape
    _chk(Ct, "Ct"); _chk(Cr, "Cr", (Nb, C, P)); _chk(stat_t, "stat_t", (2 * C,)); _chk(stat_r, "stat_r", (2 * C,), optional=True)
    out = torch.empty_like(Ct)
    call("coskad_bn2_apply_prelu_f32", Ct, Cr, stat_t, gt, bt, stat_r, gr, br, slope, out, Nb, C, P, _stream(), drop_p, drop_seed)
    return out


def dropout_mask(shape, drop_p: float, drop_seed: int, device) -> Tensor:
    """The mask bn2_apply_prelu / bn2_bwd apply for (drop_p, drop_seed): values 0 or 1 / (1 - p), in element order."""
    out = torch.empty(shape, device=device, dtype=torch.float32)
    call("coskad_dropout_mask_f32", out, out.numel(), drop_p, drop_seed, _stream())
    return out


def bn2_bwd(Ct, Cr, dOut, stat_t, gt, bt, stat_r, gr, br, slope, training: bool, drop_p: float = 0.0, drop_seed: int = 0,
            into: Optional[dict] = None):
    """-> (dCt, dCr, dgt, dbt, dgr, dbr, dslope) (residual gradients None for an identity residual).  `into`: destinations for the
    parameter gradients ('gt', 'bt', 'gr', 'br', 'slope': e.g. views of a flat gradient buffer) instead of fresh tensors."""
    Nb, C, P = Ct.shape
    _chk(dOut, "dOut", (Nb, C, P))
    into = into or {}
    dCt, dCr = torch.empty_like(Ct), torch.empty_like(Ct)
    dgt = into.get("gt") if into.get("gt") is not None else torch.empty_like(gt)
    dbt = into.get("bt") if into.get("bt") is not None else torch.empty_like(bt)
    dgr = (into.get("gr") if into.get("gr") is not None else torch.empty_like(gr)) if stat_r is not None else None
    dbr = (into.get("br") if into.get("br") is not None else torch.empty_like(br)) if stat_r is not None else None
    dslope = into.get("slope") if into.get("slope") is not None else torch.empty(1, device=Ct.device, dtype=torch.float32)
    _chk(dgt, "dgt", (C,)); _chk(dbt, "dbt", (C,)); _chk(dgr, "dgr", (C,), optional=True); _chk(dbr, "dbr", (C,), optional=True)
    _chk(dslope, "dslope", (1,))
    ws = _bn2_ws(Nb, C, Ct.device, bwd=True)
    call("coskad_bn2_bwd_f32", Ct, Cr, dOut, stat_t, gt, bt, stat_r, gr, br, slope, dCt, dCr, dgt, dbt, dgr, dbr, dslope,
         1 if training else 0, ws, ws.numel(), Nb, C, P, _stream(), drop_p, drop_seed)
    return dCt, dCr, dgt, dbt, dgr, dbr, dslope


def mlp_head_ws_floats(B: int, H: int, L: int) -> int:
    return _lib.lib().coskad_mlp_head_ws_floats(B, H, L)


def mlp_head_fwd(y1, gamma, beta, running_mean, running_var, nbt, W2, b2, training: bool, momentum: float = 0.1,
                 eps: float = 1e-5):
    """z = W2 . relu(BatchNorm1d(y1)) + b2 (the `mlp` projector behind its first Linear, components.py:209-226).
    -> (z [B,L], stat: [0:2H] = mean, invstd (the kernels' partial sums behind them)).  Train mode updates the running statistics."""
    B, H = y1.shape
    L = W2.shape[0]
    _chk(y1, "y1"); _chk(gamma, "gamma", (H,)); _chk(beta, "beta", (H,)); _chk(W2, "W2", (L, H)); _chk(b2, "b2", (L,), optional=True)
    _chk(running_mean, "running_mean", (H,), optional=True); _chk(running_var, "running_var", (H,), optional=True)
    _chk(nbt, "num_batches_tracked", (), dtype=torch.int64, optional=True)
    z = torch.empty(B, L, device=y1.device, dtype=torch.float32)
    stat = torch.empty(mlp_head_ws_floats(B, H, L), device=y1.device, dtype=torch.float32)
    if training:
        note_raw_write()
    call("coskad_mlp_head_fwd_f32", y1, gamma, beta, running_mean, running_var, nbt, momentum, eps, 1 if training else 0, W2, b2, z, stat,
         B, H, L, _stream())
    return z, stat


def mlp_head_bwd(y1, stat, gamma, beta, W2, dz, grads: dict, training: bool, accumulate: bool = False):
    """-> dy1 [B,H]; fills grads['gamma'], grads['beta'], grads['W2'] and (optional) grads['b2']."""
    B, H = y1.shape
    L = W2.shape[0]
    _chk(y1, "y1"); _chk(stat, "stat"); _chk(gamma, "gamma", (H,)); _chk(beta, "beta", (H,)); _chk(W2, "W2", (L, H))
    if stat.numel() < 2 * H:
        raise ValueError("mlp_head_bwd: stat holds fewer than 2 H values")
    _chk(dz, "dz", (B, L)); _chk(grads["gamma"], "dgamma", (H,)); _chk(grads["beta"], "dbeta", (H,)); _chk(grads["W2"], "dW2", (L, H))
    _chk(grads.get("b2"), "db2", (L,), optional=True)
    dy1 = torch.empty_like(y1)
    red = torch.empty(mlp_head_ws_floats(B, H, L), device=y1.device, dtype=torch.float32)
    call("coskad_mlp_head_bwd_f32", y1, stat, gamma, beta, W2, dz, dy1, grads["gamma"], grads["beta"], grads["W2"], grads.get("b2"), red,
         1 if training else 0, 1 if accumulate else 0, B, H, L, _stream())
    return dy1


HEAD_SLOTS = 19     # floats of a stats / acc block at latent <= 16 (head_slots(L) at any latent)


def head_slots(L: int) -> int:
    """Floats of a head's stats / acc block at latent L (coskad_head_slots_l): with Lp = max(L, 16), [0] loss term, [1..Lp] vector
    sum, [Lp+1] scalar A (clip count / sum (gamma - 1)), [Lp+2] scalar B.  HEAD_SLOTS at L <= 16."""
    if not 0 < L <= BTLNK_LMAX:
        raise ValueError(f"latent_dim={L}: the head kernels take 1 .. {BTLNK_LMAX}")
    return max(L, 16) + 3


def head_count_slot(L: int) -> int:
    """Slot of scalar A (the clip count of the Euclidean / Mahalanobis sums): Lp + 1."""
    return max(L, 16) + 1


def head_ws(B: int, device, L: int = 16) -> Tensor:
    return torch.empty(_lib.lib().coskad_head_ws_floats_l(B, L), device=device, dtype=torch.float32)


def mse_head(z, c, need_grad=True, need_score=False, acc=None, upstream=1.0, ws=None):
    """-> (stats[head_slots(L)], dz or None, score or None).  stats[0] = F.mse_loss(z, c)."""
    B, L = z.shape
    S = head_slots(L)
    _chk(z, "z"); _chk(c, "c", (L,)); _chk(acc, "acc", (S,), optional=True)
    ws = head_ws(B, z.device, L) if ws is None else ws
    dz = torch.empty_like(z) if need_grad else None
    score = torch.empty(B, device=z.device, dtype=torch.float32) if need_score else None
    stats = torch.empty(S, device=z.device, dtype=torch.float32)
    call("coskad_mse_head_f32", z, c, dz, score, stats, acc, upstream, ws, B, L, _stream())
    return stats, dz, score


def mahalanobis_head(z, c, VI, need_grad=True, need_score=False, acc=None, gram=None, gram_accumulate=True,
                     upstream=1.0, ws=None):
    """-> (stats[head_slots(L)], dz or None, score or None).  stats[0] = mahalanobis(z, c, VI) (mean); gram (+)= sum z z^T."""
    B, L = z.shape
    S = head_slots(L)
    _chk(z, "z"); _chk(c, "c", (L,)); _chk(VI, "VI", (L, L)); _chk(acc, "acc", (S,), optional=True)
    _chk(gram, "gram", (L, L), optional=True)
    ws = head_ws(B, z.device, L) if ws is None else ws
    dz = torch.empty_like(z) if need_grad else None
    score = torch.empty(B, device=z.device, dtype=torch.float32) if need_score else None
    stats = torch.empty(S, device=z.device, dtype=torch.float32)
    call("coskad_mahalanobis_head_f32", z, c, VI, dz, score, stats, acc, gram, int(gram_accumulate), upstream, ws, B, L, _stream())
    return stats, dz, score


def poincare_head(z, c, need_grad=True, need_zh=False, need_score=False, acc=None, upstream=1.0, ws=None):
    """-> (stats[head_slots(L)], dz, zh, score).  stats[0] = dist(c, project(expmap0(z))).mean()."""
    B, L = z.shape
    S = head_slots(L)
    _chk(z, "z"); _chk(c, "c", (L,), optional=True); _chk(acc, "acc", (S,), optional=True)
    ws = head_ws(B, z.device, L) if ws is None else ws
    dz = torch.empty_like(z) if (need_grad and c is not None) else None
    zh = torch.empty_like(z) if need_zh else None
    score = torch.empty(B, device=z.device, dtype=torch.float32) if (need_score and c is not None) else None
    stats = torch.empty(S, device=z.device, dtype=torch.float32)
    call("coskad_poincare_head_f32", z, c, dz, zh, score, stats, acc, upstream, ws, B, L, _stream())
    return stats, dz, zh, score


def poincare_dist(zh, c):
    B, L = zh.shape
    _chk(zh, "zh"); _chk(c, "c", (L,))
    score = torch.empty(B, device=zh.device, dtype=torch.float32)
    call("coskad_poincare_dist_f32", zh, c, score, B, L, _stream())
    return score


def poincare_logmap0(y):
    """logmap0 on the unit Poincare ball (reference utils/hyper_math.py:367-370, c = 1): tangent vector at the origin."""
    B, L = y.shape
    _chk(y, "y")
    out = torch.empty_like(y)
    call("coskad_poincare_logmap0_f32", y, out, B, L, _stream())
    return out


def lowrank_fold_ok(latent: int, TV: int) -> bool:
    return bool(_lib.lib().coskad_lowrank_fold_ok(latent, TV))


def lowrank_fold_fwd(X: Tensor, G: Tensor, bn_t, bn_r, bias_t, bias_r, n_pos: float):
    """csrc/lowrank_fold.hip: X [2, 9, Co, TV] fp32, G [9, 9] fp64 -> (Mw [Co TV, 8], Mb [Co TV], ctx); updates the running statistics of
    the two BatchNorm modules (call once per training forward)."""
    R, K, Co, TV = X.shape
    _chk(X, "X", (2, 9, Co, TV)); _chk(G, "G", (9, 9), dtype=torch.float64)
    dev = X.device
    Mw = torch.empty(Co * TV, K - 1, device=dev, dtype=torch.float32)
    Mb = torch.empty(Co * TV, device=dev, dtype=torch.float32)
    saved = torch.empty(3, 2, Co, device=dev, dtype=torch.float64)
    xbar = torch.empty(2, K, Co, device=dev, dtype=torch.float64)
    xx = torch.empty(2, Co, K, K, device=dev, dtype=torch.float64)
    args = []
    for bn, cb in ((bn_t, bias_t), (bn_r, bias_r)):
        args += [bn.weight, bn.bias, cb, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn_momentum(bn), bn.eps]
    note_raw_write()
    call("coskad_lowrank_fold_fwd_f32", X, G, *args, n_pos, Mw, Mb, saved, xbar, xx, Co, TV, _stream())
    return Mw, Mb, (saved, xbar, xx)


def lowrank_fold_bwd(X: Tensor, G: Tensor, dMw: Tensor, dMb: Tensor, ctx, gamma_t: Tensor, gamma_r: Tensor, n_pos: float):
    """-> (dX [2, 9, Co, TV], dgamma [2, Co], dbeta [Co], dG [9, 9] fp64)"""
    R, K, Co, TV = X.shape
    saved, xbar, xx = ctx
    _chk(dMw, "dMw", (Co * TV, K - 1)); _chk(dMb, "dMb", (Co * TV,))
    dev = X.device
    dX = torch.empty_like(X)
    dgamma = torch.empty(2, Co, device=dev, dtype=torch.float32)
    dbeta = torch.empty(Co, device=dev, dtype=torch.float32)
    dGc = torch.empty(Co, K, K, device=dev, dtype=torch.float64)
    call("coskad_lowrank_fold_bwd_f32", X, G, dMw, dMb, saved, xbar, xx, gamma_t, gamma_r, n_pos, dX, dgamma, dbeta, dGc, Co, TV, _stream())
    return dX, dgamma, dbeta, dGc.sum(0)


def narrow_conv_ok(Ci: int, J: int, TV: int) -> bool:
    return Ci in (16, 32, 64) and J in (2, 4, 6, 8) and TV % 4 == 0


def narrow_conv_fwd(U: Tensor, in_slope: Optional[Tensor], W: Tensor) -> Tensor:
    """[Y; R] = W . PReLU(U): U [B, Ci, T, V] (pre-activation when in_slope is given), W [J, Ci] -> [B, J, T, V] (csrc/last_layer.hip)"""
    B, Ci, T, V = U.shape
    J = W.shape[0]
    _chk(U, "U"); _chk(W, "W", (J, Ci)); _chk(in_slope, "in_slope", (1,), optional=True)
    out = torch.empty(B, J, T, V, device=U.device, dtype=torch.float32)
    call("coskad_narrow_conv_fwd_f32", U, in_slope, W, out, B, Ci, J, T * V, _stream())
    return out


def narrow_conv_bwd(U: Tensor, in_slope: Optional[Tensor], W: Tensor, dOut: Tensor):
    """-> (dU [B, Ci, T, V], sums [J Ci + 1]): dU = (W^T dOut) PReLU'(U); sums[:J Ci] = dW (row-major [J, Ci]), sums[-1] = the producer's
    slope gradient (0 without in_slope)."""
    B, Ci, T, V = U.shape
    J = W.shape[0]
    _chk(U, "U"); _chk(W, "W", (J, Ci)); _chk(dOut, "dOut", (B, J, T, V)); _chk(in_slope, "in_slope", (1,), optional=True)
    rows = _lib.lib().coskad_narrow_conv_rows(B, T * V)
    E = J * Ci + 1
    part = torch.empty(rows, E, device=U.device, dtype=torch.float32)
    dU = torch.empty_like(U)
    call("coskad_narrow_conv_bwd_f32", U, in_slope, W, dOut, dU, part, part.numel(), B, Ci, J, T * V, _stream())
    sums = torch.empty(E, device=U.device, dtype=torch.float32)
    call("coskad_gemm_sum_f32", part, rows, E, sums, 0, _stream())
    return dU, sums


def commute_ok(T: int, V: int, Ci: int, Co: int) -> bool:
    """the (C_in -> C_out) layers csrc/commute_layer.hip runs by commutation (convolutions first, mixing on C_out channels)"""
    return bool(_lib.lib().coskad_commute_ok(T, V, Ci, Co))


_commute_ws: dict = {}


def _commute_scratch(B: int, T: int, V: int, dev) -> Tensor:
    lib = _lib.lib()
    n = int(lib.coskad_commute_ws_floats(B, T, V))
    key = (str(dev), T, V)
    ws = _commute_ws.get(key)
    if ws is None or ws.numel() < n:
        ws = _commute_ws[key] = torch.empty(n, device=dev, dtype=torch.float32)
    return ws


def commute_fwd(U_prev: Tensor, in_slope: Optional[Tensor], Wt: Tensor, Wr: Tensor, A: Tensor, Tm: Tensor, gamma_t: Tensor, beta_t: Tensor,
                gamma_r: Tensor, beta_r: Tensor, bias_t: Optional[Tensor], bias_r: Optional[Tensor], rm_t: Optional[Tensor],
                rv_t: Optional[Tensor], rm_r: Optional[Tensor], rv_r: Optional[Tensor], nbt_t: Optional[Tensor],
                nbt_r: Optional[Tensor], momentum: float, eps: float, next_layer=None, slope_out: Optional[Tensor] = None):
    """Training-mode forward of a 32 -> 16 ST_GCNN layer by commutation (csrc/commute_layer.hip; reference
    models/graph_layers/stsgcn.py:94-116): U_prev [B, 32, T, V] (pre-activation when in_slope is given), Wt / Wr [16, 32(, 1, 1)] the
    two convolutions' weights -> (U [B, 16, T, V] pre-activation output, saved, pending).  next_layer = (A, T) of the layer behind
    (16 input channels) with slope_out = this layer's PReLU weight: its statistics pass rides on the last kernel and pending =
    (Z_next, partials, rows) is what engine.chain_forward takes as `pending0`; else pending is None."""
    B, Ci, T, V = U_prev.shape
    _chk(U_prev, "U_prev"); _chk(in_slope, "in_slope", (1,), optional=True)
    for n, t in (("Wt", Wt), ("Wr", Wr)):
        _cuda_f32(t, n)
        if t.numel() != 512 or not t.is_contiguous():
            raise ValueError(f"{n}: expected a contiguous [16, 32] weight")
    _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    for n, t in (("gamma_t", gamma_t), ("beta_t", beta_t), ("gamma_r", gamma_r), ("beta_r", beta_r)):
        _chk(t, n, (16,))
    for n, t in (("bias_t", bias_t), ("bias_r", bias_r), ("rm_t", rm_t), ("rv_t", rv_t), ("rm_r", rm_r), ("rv_r", rv_r)):
        _chk(t, n, (16,), optional=True)
    dev = U_prev.device
    YR = torch.empty(B, 32, T, V, device=dev, dtype=torch.float32)
    Zy = torch.empty(B, 16, T, V, device=dev, dtype=torch.float32)
    U = torch.empty(B, 16, T, V, device=dev, dtype=torch.float32)
    stat = torch.empty(128, device=dev, dtype=torch.float32)
    ws = _commute_scratch(B, T, V, dev)
    An = Tn = Zn = pn = None
    rows = ctypes.c_int(0)
    if next_layer is not None:
        An, Tn = next_layer
        _chk(An, "A_next", (T, V, V)); _chk(Tn, "T_next", (V, T, T)); _chk(slope_out, "slope_out", (1,))
        Zn = torch.empty(B, 16, T, V, device=dev, dtype=torch.float32)
        pn = torch.empty(768 * 2 * (16 * 16 + 16), device=dev, dtype=torch.float32)
    note_raw_write()
    call("coskad_commute_fwd_f32", U_prev, in_slope, Wt, Wr, A, Tm, gamma_t, beta_t, gamma_r, beta_r, bias_t, bias_r, rm_t, rv_t, rm_r,
         rv_r, nbt_t, nbt_r, momentum, eps, YR, Zy, U, stat, ws, ws.numel(), An, Tn, slope_out if next_layer is not None else None, Zn, pn,
         ctypes.byref(rows), B, T, V, _stream())
    pending = (Zn, pn, int(rows.value)) if next_layer is not None else None
    return U, (U_prev, in_slope, Wt, Wr, A, Tm, YR, Zy, stat), pending


def commute_bwd(saved, dU: Tensor, into: dict, below=None):
    """-> (gradient of U_prev [B, 32, T, V] (PReLU mask applied), chain).  below = (x_below [B, 2, T, V], Z_below) of a 2-channel layer
    in front (the first layer, fed by the network input): its batch reductions are formed by the same kernel and chain = (buffer, rows) is
    what engine.chain_backward takes as `stats_in`; else chain is None.  `into`: destinations (all overwritten) 'A' [T, V, V], 'T' [V, T, T],
    'Wt' / 'Wr' [16, 32(, 1, 1)], 'gt' 'bet' 'gr' 'ber' [16], 'in_slope' [1] (the producer's PReLU weight gradient; with in_slope)."""
    U_prev, in_slope, Wt, Wr, A, Tm, YR, Zy, stat = saved
    B, Ci, T, V = U_prev.shape
    _chk(dU, "dU", (B, 16, T, V))
    for n, shp in (("A", (T, V, V)), ("T", (V, T, T)), ("gt", (16,)), ("bet", (16,)), ("gr", (16,)), ("ber", (16,))):
        _chk(into[n], "into." + n, shp)
    for n in ("Wt", "Wr"):
        _cuda_f32(into[n], "into." + n)
        if into[n].numel() != 512 or not into[n].is_contiguous():
            raise ValueError(f"into.{n}: expected a contiguous [16, 32] gradient view")
    dsl = into.get("in_slope") if in_slope is not None else None
    if in_slope is not None:
        _chk(dsl, "into.in_slope", (1,))
    d_in = torch.empty_like(U_prev)
    ws = _commute_scratch(B, T, V, U_prev.device)
    bx = bz = buf = None
    rows = 0
    if below is not None:
        bx, bz = below
        _chk(bx, "below.x", (B, 2, T, V)); _chk(bz, "below.Z", (B, 2, T, V))
        lib = _lib.lib()
        rows = int(lib.coskad_commute_below_rows(B))
        buf = torch.empty(int(lib.coskad_commute_below_floats(B)), device=U_prev.device, dtype=torch.float32)
    call("coskad_commute_bwd_f32", U_prev, in_slope, Wt, Wr, A, Tm, YR, Zy, stat, dU, d_in, into["A"], into["T"], into["Wt"], into["Wr"],
         into["gt"], into["bet"], into["gr"], into["ber"], dsl, ws, ws.numel(), bx, bz, buf, buf.numel() if buf is not None else 0, B, T, V,
         _stream())
    return d_in, ((buf, rows) if below is not None else None)


def _rows(t: Tensor, name: str, cols: int):
    """a [B, cols] fp32 device view with unit column stride (a column block of a wider row-major tensor is fine) -> its row stride"""
    _cuda_f32(t, name)
    if t.dim() != 2 or t.shape[1] != cols or (cols > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected a [B, {cols}] view with contiguous columns, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0)


PS_HEAD_LMAX = 512          # widest latent of the PowerSpherical head (csrc/vae_head.hip: a thread per clip to 16, a wave above)


def ps_head_forward(mean_raw: Tensor, var_raw: Tensor, generator=None):
    """The spherical VAE's latent head on csrc/vae_head.hip (2 <= L <= PS_HEAD_LMAX; reference models/sts/vae.py:79-91,104-118; PowerSpherical restated in
    coskad_amd/models/sts/vae.py): mean_raw [B, L], var_raw [B, 1] (views of one tensor are fine) -> (z [B, L] sampled latent,
    kl [B], inv_kappa [B], saved) with saved = what ps_head_backward needs.  The Beta draw and the Gaussian direction are torch's
    (torch._sample_dirichlet, torch.randn): the noise streams are the module path's."""
    B, L = mean_raw.shape
    ldm, ldv = _rows(mean_raw, "mean_raw", L), _rows(var_raw, "var_raw", 1)
    dev = mean_raw.device
    mu = torch.empty(B, L, device=dev, dtype=torch.float32)
    kappa = torch.empty(B, device=dev, dtype=torch.float32)
    conc = torch.empty(B, 2, device=dev, dtype=torch.float32)
    total = torch.empty(B, device=dev, dtype=torch.float32)
    call("coskad_ps_head_prep_f32", mean_raw, ldm, var_raw, ldv, mu, kappa, conc, total, B, L, _stream())
    x = torch._sample_dirichlet(conc, generator) if generator is not None else torch._sample_dirichlet(conc)
    eps = torch.randn(B, L - 1, device=dev, dtype=torch.float32, generator=generator)
    z = torch.empty(B, L, device=dev, dtype=torch.float32)
    kl = torch.empty(B, device=dev, dtype=torch.float32)
    ik = torch.empty(B, device=dev, dtype=torch.float32)
    call("coskad_ps_head_sample_f32", x, eps, mu, kappa, z, kl, ik, B, L, _stream())
    return z, kl, ik, (mean_raw, var_raw, mu, kappa, conc, total, x, eps)


def dirichlet_grad(x: Tensor, conc: Tensor, total: Tensor, f64: bool) -> Tensor:
    """torch._dirichlet_grad, the Beta draw's implicit reparameterisation gradient.  f64 (the callers ask at a latent beyond 16):
    evaluated in float64.  In float32 on the device (no wider accumulator there, unlike torch's CPU kernel) it is off from the
    float64 value by 0.5 % at the total concentration of latent 16, 5 % at 17, 12 % at 200 and 62 % at 512."""
    if not f64:
        return torch._dirichlet_grad(x, conc, total)
    return torch._dirichlet_grad(x.double(), conc.double(), total.double()).to(x.dtype)


def ps_head_backward(saved, dz: Tensor, w_kl: float, w_exp: float, d_mean_raw: Optional[Tensor] = None,
                     d_var_raw: Optional[Tensor] = None):
    """-> (d_mean_raw [B, L], d_var_raw [B, 1]) for loss = <dz, z> + w_kl * sum kl + w_exp * sum inv_kappa; the destinations may be
    column views of one [B, L + 1] tensor."""
    mean_raw, var_raw, mu, kappa, conc, total, x, eps = saved
    B, L = mean_raw.shape
    _chk(dz, "dz", (B, L))
    g = dirichlet_grad(x, conc, total.unsqueeze(-1).expand(B, 2).contiguous(), f64=L > 16)
    if d_mean_raw is None:
        d_mean_raw = torch.empty(B, L, device=dz.device, dtype=torch.float32)
    if d_var_raw is None:
        d_var_raw = torch.empty(B, 1, device=dz.device, dtype=torch.float32)
    call("coskad_ps_head_bwd_f32", dz, x, g, eps, mu, kappa, mean_raw, _rows(mean_raw, "mean_raw", L), var_raw,
         _rows(var_raw, "var_raw", 1), w_kl, w_exp, d_mean_raw, _rows(d_mean_raw, "d_mean_raw", L), d_var_raw,
         _rows(d_var_raw, "d_var_raw", 1), B, L, _stream())
    return d_mean_raw, d_var_raw


NORMAL_HEAD_LMAX = 512      # widest latent of the Gaussian head (csrc/vae_head_normal.hip)
# (projector, latent) ranges that a measurement found no faster on the Gaussian head's kernels than under the local autograd graph
# stay on trainer._AutogradLatent (the idiom of AE_WIDE_OFF): entries (projector, first latent, last latent).  None
NORMAL_HEAD_OFF = frozenset()


def normal_head_ok(L: int) -> bool:
    """Host arithmetic of `coskad_normal_head_ok`: the Gaussian head's kernels take the latent (1 .. NORMAL_HEAD_LMAX).  Restated here
    so that building a train step needs no native library; tests/test_gaussian_head_host.py holds the two in agreement."""
    return 1 <= L <= NORMAL_HEAD_LMAX


def normal_head_forward(mean_raw: Tensor, var_raw: Tensor, generator=None, ref: Optional[Tensor] = None, need_saved: bool = True,
                        eps: Optional[Tensor] = None):
    """The Gaussian VAE's latent head in one launch of csrc/vae_head_normal.hip (1 <= L <= NORMAL_HEAD_LMAX; reference
    models/sts/vae.py:85,106-108,129, loss terms of models/spherical_vae.py:89-90,98): mean_raw [B, L], var_raw [B, L] (column blocks of
    one tensor are fine) -> (z [B, L] = mean_raw + sigma eps, kl [B] = KL(Normal(mean_raw, sigma) || Normal(0, 1)) summed over the
    latent, inv [B] = sum_l 1 / sigma, saved) with sigma = softplus(var_raw) + 1 and saved = (mean_raw, var_raw, eps, sigma, z), what
    normal_head_backward needs (None without `need_saved`: sigma is then not written).
    ref [L] or [1, L]: the scoring form -> (score [B] = 1 - F.cosine_similarity(ref, z), kl, inv, saved); without `need_saved` only
    the score is formed (z, sigma, kl and inv are not written: None).
    eps: the noise [B, L]; None: drawn as Normal.rsample draws it (torch.distributions.utils._standard_normal: ONE
    torch.empty(shape).normal_() of shape [B, L] on the input's device), so the module path's noise stream is kept."""
    B, L = mean_raw.shape
    ldm, ldv = _rows(mean_raw, "mean_raw", L), _rows(var_raw, "var_raw", L)
    if var_raw.shape[0] != B:
        raise ValueError(f"var_raw: expected {B} rows, got {var_raw.shape[0]}")
    dev = mean_raw.device
    if eps is None:
        eps = torch.empty(B, L, device=dev, dtype=torch.float32).normal_(generator=generator)
    _chk(eps, "eps", (B, L))
    scoring = ref is not None
    if scoring:
        ref = ref.reshape(-1)
        _chk(ref, "ref", (L,))
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    full = need_saved or not scoring
    z = new(B, L) if full else None
    sigma = new(B, L) if need_saved else None
    kl, inv = (new(B), new(B)) if full else (None, None)
    score = new(B) if scoring else None
    call("coskad_normal_head_fwd_f32", mean_raw, ldm, var_raw, ldv, eps, z, sigma, kl, inv, ref, score, B, L, _stream())
    saved = (mean_raw, var_raw, eps, sigma, z) if need_saved else None
    return (score if scoring else z), kl, inv, saved


def normal_head_backward(saved, dz: Tensor, w_kl: float, w_exp: float, d_mean_raw: Optional[Tensor] = None,
                         d_var_raw: Optional[Tensor] = None):
    """-> (d_mean_raw [B, L], d_var_raw [B, L]) for loss = <dz, z> + w_kl * sum kl + w_exp * sum inv, in one launch; the destinations
    may be the column blocks of one [B, 2L] tensor."""
    mean_raw, var_raw, eps, sigma, _ = saved
    B, L = mean_raw.shape
    _chk(dz, "dz", (B, L))
    if d_mean_raw is None:
        d_mean_raw = torch.empty(B, L, device=dz.device, dtype=torch.float32)
    if d_var_raw is None:
        d_var_raw = torch.empty(B, L, device=dz.device, dtype=torch.float32)
    for t, name in ((d_mean_raw, "d_mean_raw"), (d_var_raw, "d_var_raw")):
        if t.shape[0] != B:
            raise ValueError(f"{name}: expected {B} rows, got {t.shape[0]}")
    call("coskad_normal_head_bwd_f32", dz, eps, sigma, mean_raw, _rows(mean_raw, "mean_raw", L), var_raw, _rows(var_raw, "var_raw", L),
         w_kl, w_exp, d_mean_raw, _rows(d_mean_raw, "d_mean_raw", L), d_var_raw, _rows(d_var_raw, "d_var_raw", L), B, L, _stream())
    return d_mean_raw, d_var_raw


def center_finalize(acc, eps: float, L: int):
    _chk(acc, "acc", (head_slots(L),))
    c = torch.empty(L, device=acc.device, dtype=torch.float32)
    call("coskad_center_finalize_f32", acc, c, eps, L, _stream())
    return c


def midpoint_finalize(acc, L: int):
    _chk(acc, "acc", (head_slots(L),))
    c = torch.empty(L, device=acc.device, dtype=torch.float32)
    call("coskad_midpoint_finalize_f32", acc, c, L, _stream())
    return c


def sqnorm(p, mask, scale: float, ws=None):
    _chk(p, "p"); _chk(mask, "mask", p.shape, optional=True)
    ws = torch.empty(256, device=p.device, dtype=torch.float32) if ws is None else ws
    out = torch.empty(1, device=p.device, dtype=torch.float32)
    call("coskad_sqnorm_f32", p, mask, p.numel(), scale, out, ws, _stream())
    return out


def adam(p, g, m, v, mask, lr, beta1, beta2, eps, step, gscale=1.0, reg_coef=0.0):
    for n, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, n, p.shape)
    _chk(mask, "mask", p.shape, optional=True)
    note_raw_write()
    call("coskad_adam_f32", p, g, m, v, mask, p.numel(), lr, beta1, beta2, eps, step, gscale, reg_coef, _stream())


def adam_pow(p, g, m, v, mask, lr, beta1, beta2, eps, b1pow, b2pow, gscale=1.0, reg_coef=0.0):
    """Adam with the caller's fp32 running products beta^t (the arithmetic of adam_dev's device-side tick)."""
    for n, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, n, p.shape)
    _chk(mask, "mask", p.shape, optional=True)
    note_raw_write()
    call("coskad_adam_pow_f32", p, g, m, v, mask, p.numel(), lr, beta1, beta2, eps, b1pow, b2pow, gscale, reg_coef, _stream())


def prelu_fwd(u: Tensor, slope: Tensor) -> Tensor:
    _chk(u, "u"); _chk(slope, "slope", (1,))
    out = torch.empty_like(u)
    call("coskad_prelu_fwd_f32", u, slope, out, u.numel(), _stream())
    return out


def prelu_bwd(u: Tensor, dout: Tensor, slope: Tensor, dslope: Optional[Tensor] = None, accumulate=False) -> Tensor:
    _chk(u, "u"); _chk(dout, "dout", u.shape); _chk(slope, "slope", (1,)); _chk(dslope, "dslope", (1,), optional=True)
    du = torch.empty_like(u)
    ws = torch.empty(1024, device=u.device, dtype=torch.float32)
    call("coskad_prelu_bwd_f32", u, dout, slope, du, dslope, ws, 1 if accumulate else 0, u.numel(), _stream())
    return du


def rec_head(U: Tensor, x: Tensor, slope: Tensor, need_grad: bool = True, need_xrec: bool = False, dslope: Optional[Tensor] = None,
             upstream: float = 1.0, accumulate: bool = False):
    """-> (loss [1] = F.mse_loss(PReLU(U), x), dU or None, x_rec or None); dslope (+)= the slope gradient."""
    _chk(U, "U"); _chk(x, "x", U.shape); _chk(slope, "slope", (1,)); _chk(dslope, "dslope", (1,), optional=True)
    dU = torch.empty_like(U) if need_grad else None
    xrec = torch.empty_like(U) if need_xrec else None
    loss = torch.empty(1, device=U.device, dtype=torch.float32)
    ws = torch.empty(2048, device=U.device, dtype=torch.float32)
    call("coskad_rec_head_f32", U, x, slope, xrec, dU, loss, dslope if need_grad else None, upstream, ws, 1 if accumulate else 0, U.numel(),
         _stream())
    return loss, dU, xrec


def rev_btlnk_ok(N: int, L: int) -> bool:
    return L in (8, 16) and N % 4 == 0


def rev_btlnk_wide_ok(N: int, L: int) -> bool:
    """coskad_rev_btlnk_wide_ok: the latent takes the three MFMA GEMMs of csrc/rev_btlnk_wide.hip (16 < L <= 512, N % 4 == 0)"""
    return 16 < L <= 512 and N > 0 and N % 4 == 0


# latent sizes above 16 that the decoder models' flat step (trainer.STSAETrainStep.supports) leaves on the autograd route because a
# measurement found the step no faster there (the idiom of TRAIN_WINDOW_OFF)
AE_WIDE_OFF = frozenset()
# latent sizes above 16 at which a product of rev_btlnk keeps the strided-GEMM fallback because the wide kernel did not beat it
# (DESIGN 5.19): {'fwd' | 'bwd': set of L}; the backward's two products share one entry point and move together
REV_WIDE_FALLBACK = {'fwd': frozenset(), 'bwd': frozenset()}


def rev_btlnk_fwd(z: Tensor, W: Tensor, bias: Optional[Tensor]) -> Tensor:
    """H = z W^T + bias (rev_btlnk, ae.py:223-227): one streaming pass (csrc/rev_btlnk.hip) at latent 8 / 16, an MFMA GEMM with the
    bias in its epilogue (csrc/rev_btlnk_wide.hip) at 17 .. 512; other latent sizes: the strided GEMM."""
    B, L = z.shape
    N = W.shape[0]
    _chk(z, "z"); _chk(W, "W", (N, L)); _chk(bias, "bias", (N,), optional=True)
    wide = rev_btlnk_wide_ok(N, L) and L not in REV_WIDE_FALLBACK['fwd']
    if not (rev_btlnk_ok(N, L) or wide):
        return gemm(z, W.t(), bias=bias, bias_mode=2 if bias is not None else 0)
    H = torch.empty(B, N, device=z.device, dtype=torch.float32)
    call("coskad_rev_btlnk_fwd_f32", z, W, bias, H, B, N, L, _stream())
    return H


def _rev_btlnk_bwd_gemm(dH, z, W, dW, db, dz, accumulate):
    """the products of rev_btlnk's backward on the strided GEMM (a ones column behind z gives db)"""
    B, N = dH.shape
    L = z.shape[1]
    zs1 = torch.cat([z, torch.ones(B, 1, device=z.device)], 1)
    gw = torch.empty(N, L + 1, device=dH.device, dtype=torch.float32)
    gemm_rows_outer(dH, zs1, gw)
    if accumulate:
        dW.add_(gw[:, :-1])
        if db is not None:
            db.add_(gw[:, -1])
    else:
        dW.copy_(gw[:, :-1])
        if db is not None:
            db.copy_(gw[:, -1])
    if dz is None:
        return gemm(dH, W)
    return gemm(dH, W, out=dz, accumulate=True)


def rev_btlnk_bwd(dH: Tensor, z: Tensor, W: Tensor, dW: Tensor, db: Optional[Tensor], dz: Optional[Tensor] = None,
                  accumulate: bool = False) -> Tensor:
    """-> dz [B, L] (added to the given `dz` when one is passed); fills dW [N, L] and db [N] ((+)= with `accumulate`)."""
    B, N = dH.shape
    L = z.shape[1]
    _chk(dH, "dH"); _chk(z, "z", (B, L)); _chk(W, "W", (N, L)); _chk(dW, "dW", (N, L)); _chk(db, "db", (N,), optional=True)
    _chk(dz, "dz", (B, L), optional=True)
    wide = rev_btlnk_wide_ok(N, L) and L not in REV_WIDE_FALLBACK['bwd']
    if not wide and (not rev_btlnk_ok(N, L) or dH.data_ptr() % 16):
        return _rev_btlnk_bwd_gemm(dH, z, W, dW, db, dz, accumulate)
    ws = torch.empty(_lib.lib().coskad_rev_btlnk_ws_floats(B, N, L), device=dH.device, dtype=torch.float32)
    acc_dz = dz is not None
    if dz is None:
        dz = torch.empty(B, L, device=dH.device, dtype=torch.float32)
    call("coskad_rev_btlnk_bwd_f32", dH, z, W, dz, 1 if acc_dz else 0, dW, db, 1 if accumulate else 0, ws, B, N, L, _stream())
    return dz


def gcn_bwd_params(x: Tensor, dZ: Tensor, A: Tensor, Tm: Tensor):
    """(dA, dT) of ConvTemporalGraphical given its input and output gradient."""
    N, C, T, V = x.shape
    _chk(x, "x"); _chk(dZ, "dZ", x.shape); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T))
    nbytes = _lib.lib().coskad_gcn_bwd_params_ws_bytes(T, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    dA, dT = torch.empty_like(A), torch.empty_like(Tm)
    call("coskad_gcn_bwd_params_f32", x, dZ, A, Tm, dA, dT, ws, nbytes, 0, N * C, T, V, _stream())
    return dA, dT


def gcn_bwd_params_dx(x: Tensor, dZ: Tensor, A: Tensor, Tm: Tensor, add: Optional[Tensor] = None, dA: Optional[Tensor] = None,
                      dT: Optional[Tensor] = None, accumulate: bool = False):
    """(dA, dT, dX) of ConvTemporalGraphical in one pass over dZ: dX = gcn^T(dZ) (+ add, e.g. an identity residual's gradient);
    dA / dT: destinations (e.g. views of a flat gradient buffer) instead of fresh tensors; accumulate: add to them."""
    N, C, T, V = x.shape
    _chk(x, "x"); _chk(dZ, "dZ", x.shape); _chk(A, "A", (T, V, V)); _chk(Tm, "T", (V, T, T)); _chk(add, "add", x.shape, optional=True)
    nbytes = _lib.lib().coskad_gcn_bwd_params_ws_bytes(T, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    if accumulate and (dA is None or dT is None):
        raise ValueError("gcn_bwd_params_dx: accumulate needs the dA and dT to add to")
    dA = torch.empty_like(A) if dA is None else dA
    dT = torch.empty_like(Tm) if dT is None else dT
    _chk(dA, "dA", (T, V, V)); _chk(dT, "dT", (V, T, T))
    dX = torch.empty_like(x)
    call("coskad_gcn_bwd_params_dx_f32", x, dZ, A, Tm, dA, dT, dX, add, ws, nbytes, 1 if accumulate else 0, N * C, T, V, _stream())
    return dA, dT, dX


def adam_dev(p, g, m, v, mask, hyper, beta1, beta2, eps, gscale=1.0, reg_coef=0.0):
    """Adam with {lr, beta1^t, beta2^t} in the device tensor `hyper` (replayable in a hipGraph)."""
    for n, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, n, p.shape)
    _chk(mask, "mask", p.shape, optional=True); _chk(hyper, "hyper", (4,))
    note_raw_write()
    call("coskad_adam_dev_f32", p, g, m, v, mask, p.numel(), hyper, beta1, beta2, eps, gscale, reg_coef, _stream())


CLIP_PARTIALS = 256            # fp64 entries of grad_sqnorm's partials (csrc/grad_clip.hip: kClipPartials)
CLIP_MODES = {'norm': 1, 'value': 2}


def grad_sqnorm(g, p, mask, gscale=1.0, reg_coef=0.0, partials=None):
    """partials [256] float64 whose sum is |g * gscale + reg_coef * mask * p|^2, the gradient Adam applies (fixed order: repeated
    calls agree bit for bit); adam_clip_pow / adam_clip_dev read them."""
    _chk(g, "g"); _chk(p, "p", g.shape); _chk(mask, "mask", g.shape, optional=True)
    if partials is None:
        partials = torch.empty(CLIP_PARTIALS, device=g.device, dtype=torch.float64)
    _chk(partials, "partials", (CLIP_PARTIALS,), dtype=torch.float64)
    call("coskad_grad_sqnorm_f32", g, p, mask, g.numel(), gscale, reg_coef, partials, _stream())
    return partials


def _chk_clip(p, g, m, v, mask, partials, mode, norm_out) -> int:
    for n, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, n, p.shape)
    _chk(mask, "mask", p.shape, optional=True)
    if mode not in CLIP_MODES:
        raise ValueError(f"clip mode {mode!r}: one of {sorted(CLIP_MODES)}")
    _chk(partials, "partials", (CLIP_PARTIALS,), dtype=torch.float64, optional=mode == 'value')
    _chk(norm_out, "norm_out", (1,), optional=True)
    return CLIP_MODES[mode]


def adam_clip_pow(p, g, m, v, mask, lr, beta1, beta2, eps, b1pow, b2pow, partials, clip_val, mode='norm', norm_out=None,
                  gscale=1.0, reg_coef=0.0):
    """adam_pow with the applied gradient clipped: mode 'norm' by the global norm behind grad_sqnorm's `partials` (the unclipped
    norm goes to norm_out [1]), mode 'value' by clamping to [-clip_val, clip_val] (no partials)."""
    k = _chk_clip(p, g, m, v, mask, partials, mode, norm_out)
    note_raw_write()
    call("coskad_adam_clip_pow_f32", p, g, m, v, mask, p.numel(), lr, beta1, beta2, eps, b1pow, b2pow, gscale, reg_coef, partials,
         clip_val, k, norm_out, _stream())


def adam_clip_dev(p, g, m, v, mask, hyper, beta1, beta2, eps, partials, clip_val, mode='norm', norm_out=None, gscale=1.0,
                  reg_coef=0.0):
    """adam_dev with the same clipping ({lr, beta1^t, beta2^t} in the device tensor `hyper`: replayable in a hipGraph)."""
    k = _chk_clip(p, g, m, v, mask, partials, mode, norm_out)
    _chk(hyper, "hyper", (4,))
    note_raw_write()
    call("coskad_adam_clip_dev_f32", p, g, m, v, mask, p.numel(), hyper, beta1, beta2, eps, gscale, reg_coef, partials, clip_val, k,
         norm_out, _stream())


def grad_accum(acc, g, first: bool):
    """acc = g (first) or acc + g: the gradient sum over the micro-batches of one accumulation group"""
    _chk(acc, "acc"); _chk(g, "g", acc.shape)
    call("coskad_grad_accum_f32", acc, g, acc.numel(), 1 if first else 0, _stream())
    return acc


def gather_transform(xy, mats, index, T, V):
    """Batch [B, 2, T, V] from the device-resident window table xy [N, 2, T*V]: item i = transform i // N of window
    i % N (utils/dataset.py:65-77; PoseTransform of utils/dataset_utils.py:272-310)."""
    N = xy.shape[0]
    _chk(xy, "xy", (N, 2, T * V)); _chk(mats, "mats", (mats.shape[0], 3, 3)); _chk(index, "index", dtype=torch.int64)
    B = index.numel()
    out = torch.empty(B, 2, T, V, device=xy.device, dtype=torch.float32)
    call("coskad_gather_transform_f32", xy, index, mats, out, B, N, mats.shape[0], T * V, _stream())
    return out


def gather_frames(fxy, win_row, mats, index, T, V, step):
    """The same batch [B, 2, T, V] from the device-resident FRAME table fxy [F, 2, V] (one row per trajectory frame): window s is
    the rows win_row[s] + t * step, t < T; item i = transform i // N of window i % N with N = win_row.numel().  An index outside
    [0, N * ntrans) and a window whose rows leave the table give a zero clip."""
    F, N = fxy.shape[0], win_row.numel()
    _chk(fxy, "fxy", (F, 2, V)); _chk(win_row, "win_row", (N,), dtype=torch.int32)
    _chk(mats, "mats", (mats.shape[0], 3, 3)); _chk(index, "index", dtype=torch.int64)
    B = index.numel()
    out = torch.empty(B, 2, T, V, device=fxy.device, dtype=torch.float32)
    call("coskad_gather_frames_f32", fxy, win_row, index, mats, out, B, N, F, mats.shape[0], T, V, step, _stream())
    return out


# ---- frame-level scoring of a validation pass (csrc/score_frames.hip; tables from utils/score_plan.ScorePlan) ----

def score_person_frames(scores, win_ptr, win_idx):
    """pf [win_ptr.numel() - 1] float64: per (person, frame) the mean of the covering windows' scores that are not exactly 0
    (0 when none is left); scores float32 or float64, widened on load."""
    if scores.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"scores: expected float32 or float64, got {scores.dtype}")
    _chk(scores, "scores", dtype=scores.dtype); _chk(win_ptr, "win_ptr", dtype=torch.int32); _chk(win_idx, "win_idx", dtype=torch.int32)
    rows = win_ptr.numel() - 1
    pf = torch.empty(rows, device=scores.device, dtype=torch.float64)
    call("coskad_score_person_frames_f64", scores, int(scores.dtype == torch.float64), win_ptr, win_idx, pf, scores.numel(), rows, _stream())
    return pf


def attribution_frames(attr, frames, win_ptr, win_idx, entry_frame):
    """out [win_ptr.numel() - 1, V] float64: per (person, frame) the mean over the covering windows of the row attr[w, t] with
    frames[w, t] == entry_frame[row] (attr [N, T, V] float32, frames [N, T] int32); NaN where no window holds the frame."""
    N, T, V = attr.shape
    rows = win_ptr.numel() - 1
    _chk(attr, "attr"); _chk(frames, "frames", (N, T), dtype=torch.int32); _chk(win_ptr, "win_ptr", dtype=torch.int32)
    _chk(win_idx, "win_idx", dtype=torch.int32); _chk(entry_frame, "entry_frame", (rows,), dtype=torch.int32)
    out = torch.empty(rows, V, device=attr.device, dtype=torch.float64)
    call("coskad_attribution_frames_f64", attr, frames, win_ptr, win_idx, entry_frame, out, N, rows, T, V, _stream())
    return out


def score_pad_(pf, row_ptr, pad_size, n_max):
    """pad_scores (utils/eval_utils.py:232-248) on every person's row pf[row_ptr[p] : row_ptr[p + 1]], in place."""
    _chk(pf, "pf", dtype=torch.float64); _chk(row_ptr, "row_ptr", dtype=torch.int32)
    call("coskad_score_pad_f64", pf, row_ptr, row_ptr.numel() - 1, pad_size, n_max, _stream())
    return pf


def score_clip_max(pf, row_ptr, pc_ptr, out_clip, out_frame, n_clips, n_transform):
    """raw [n_transform, F] float64: max over each clip's persons, gathered into the concatenated output layout."""
    _chk(pf, "pf", dtype=torch.float64)
    for n, t in (("row_ptr", row_ptr), ("pc_ptr", pc_ptr), ("out_clip", out_clip), ("out_frame", out_frame)):
        _chk(t, n, dtype=torch.int32)
    _chk(pc_ptr, "pc_ptr", (n_transform * n_clips + 1,), dtype=torch.int32); _chk(out_frame, "out_frame", out_clip.shape, dtype=torch.int32)
    F = out_clip.numel()
    raw = torch.empty(n_transform, F, device=pf.device, dtype=torch.float64)
    call("coskad_score_clip_max_f64", pf, row_ptr, pc_ptr, out_clip, out_frame, raw, n_clips, n_transform, F, _stream())
    return raw


def score_smooth(raw, tiles, taps):
    """Shift by 11 and gaussian_filter1d(sigma 30, reflect) per clip segment: raw [n_transform, F] -> (per_t [n_transform, F],
    mean over the transformations [F]); tiles [n_tiles, 3] = (segment start, segment end, tile start)."""
    _chk(raw, "raw", dtype=torch.float64); _chk(tiles, "tiles", (tiles.shape[0], 3), dtype=torch.int32); _chk(taps, "taps", dtype=torch.float64)
    nt, F = raw.shape
    per_t, mean = torch.empty_like(raw), torch.empty(F, device=raw.device, dtype=torch.float64)
    call("coskad_score_smooth_f64", raw, tiles, taps, taps.numel(), per_t, mean, tiles.shape[0], nt, F, _stream())
    return per_t, mean


def score_auc(sorted_scores, gt_sorted, cum_neg):
    """[AUC, n_pos, n_neg] float64 on the device from ascending scores, the ground truth in that order (int32, non-zero = positive) and
    its inclusive count of negatives (int64): the tie-aware Mann-Whitney statistic, formed in int64.  AUC is NaN for a single class."""
    F = sorted_scores.numel()
    _chk(sorted_scores, "sorted_scores", dtype=torch.float64); _chk(gt_sorted, "gt_sorted", (F,), dtype=torch.int32)
    _chk(cum_neg, "cum_neg", (F,), dtype=torch.int64)
    out = torch.empty(3, device=sorted_scores.device, dtype=torch.float64)
    ws = torch.empty(max(1, _lib.lib().coskad_score_auc_ws(F)), device=sorted_scores.device, dtype=torch.int64)
    call("coskad_score_auc_f64", sorted_scores, gt_sorted, cum_neg, out, ws, ws.numel(), F, _stream())
    return out


# ---- the evaluation report (csrc/score_report.hip): per-segment AUCs and ROC thresholds of rows ordered by the caller ----

REPORT_TILE = 256                   # elements per workgroup of the report kernels (coskad_score_report_tile())


def score_report_auc(sorted_scores, gt_sorted, cum_neg, segments, tile_ptr, n_tiles, out=None):
    """out [n_rows, n_seg, 3] float64 = {AUC, n_pos, n_neg} of every segment [start, end) (int32 [n_seg, 2], not overlapping) of every
    row: sorted_scores [n_rows, F] ascending inside each segment, gt_sorted in that order (int32), cum_neg its inclusive count of
    negatives along the row (int64); tile_ptr [n_seg + 1] int32 the running sum of the segments' tile counts, n_tiles >= its last entry.
    Two launches whatever n_seg; AUC is NaN for a segment of one class or without frames."""
    _chk(sorted_scores, "sorted_scores", dtype=torch.float64)
    if sorted_scores.dim() != 2:
        raise ValueError(f"sorted_scores: expected [n_rows, F], got {tuple(sorted_scores.shape)}")
    R, F = sorted_scores.shape
    _chk(gt_sorted, "gt_sorted", (R, F), dtype=torch.int32); _chk(cum_neg, "cum_neg", (R, F), dtype=torch.int64)
    S = segments.shape[0]
    _chk(segments, "segments", (S, 2), dtype=torch.int32); _chk(tile_ptr, "tile_ptr", (S + 1,), dtype=torch.int32)
    if out is None:
        out = torch.empty(R, S, 3, device=sorted_scores.device, dtype=torch.float64)
    else:
        _chk(out, "out", (R, S, 3), dtype=torch.float64)
    ws = torch.empty(max(1, R * n_tiles), device=sorted_scores.device, dtype=torch.int64)
    call("coskad_score_report_auc_f64", sorted_scores, gt_sorted, cum_neg, segments, tile_ptr, out, ws, ws.numel(), n_tiles, R, S, F,
         _stream())
    return out


def score_report_thresholds(sorted_scores, cum_neg, out=None):
    """out [n_rows, 3] float64 = {n, thr0, thr1}: the n thresholds (1 or 2; 0 for a single-class row) at which the ROC curve of each row
    crosses tpr = 1 - fpr, as sklearn's roc_curve (drop_intermediate=True) and the reference's ROC() give them; sorted_scores [n_rows, F]
    ascending along each row, cum_neg the inclusive count of negatives in that order (int64).  Two launches."""
    _chk(sorted_scores, "sorted_scores", dtype=torch.float64)
    if sorted_scores.dim() != 2:
        raise ValueError(f"sorted_scores: expected [n_rows, F], got {tuple(sorted_scores.shape)}")
    R, F = sorted_scores.shape
    _chk(cum_neg, "cum_neg", (R, F), dtype=torch.int64)
    if out is None:
        out = torch.empty(R, 3, device=sorted_scores.device, dtype=torch.float64)
    else:
        _chk(out, "out", (R, 3), dtype=torch.float64)
    ws = torch.empty(max(1, 2 * R * ((F + REPORT_TILE - 1) // REPORT_TILE)), device=sorted_scores.device, dtype=torch.int32)
    call("coskad_score_report_thresholds_f64", sorted_scores, cum_neg, out, ws, ws.numel(), R, F, _stream())
    return out


# ---- online scoring of live pose tracks (csrc/stream.hip; bookkeeping and the public class in coskad_amd/stream.py) ----

STREAM_WINDOWS = (8, 12, 16, 24)    # window lengths of the stream kernels
STREAM_JOINTS = (14, 17, 18)        # headless, plain, kp18_format
STREAM_KP18, STREAM_HEADLESS, STREAM_NORMALISED = 1, 2, 4       # layout flags of coskad_stream_push_f32


def stream_ok(T: int, V: int) -> bool:
    """Host arithmetic of `coskad_stream_ok`: the stream kernels take windows of T frames and V joints.  Restated here so that the
    bookkeeping of coskad_amd/stream.py needs no native library; tests/test_stream_host.py holds the two in agreement."""
    return T in STREAM_WINDOWS and V in STREAM_JOINTS


def stream_rows(T: int, step: int) -> int:
    """R = (T - 1) step + 1: the rows from a window's first to its last, the length of a track's rings"""
    return (T - 1) * step + 1


def _chk_host_i32(t: Tensor, name: str, n: int) -> None:
    if t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{name}: expected {n} contiguous int32 values on the host")


def stream_push(raw, slot, slot_host, reset, out_index, center, scale, vid_res, flags, mats, ring, count, m, T, V, step):
    """One frame of detections into the tracks' rings, and the K transformed copies of every window that became full
    (`coskad_stream_push_f32`): raw [n, 34] f32 pixel rows, slot / reset / out_index [n] int32 on the device, slot_host the host's copy
    of `slot`, center / scale [34] f64 or None, vid_res (width, height) or None with STREAM_NORMALISED, mats [K, 3, 3], ring
    [M, R, 2, V], count [M].  -> x_out [K m, 2, T, V] (None at m = 0)."""
    n, M, K = raw.shape[0], count.numel(), mats.shape[0]
    R = stream_rows(T, step)
    _chk(raw, "raw", (n, 34)); _chk(mats, "mats", (K, 3, 3)); _chk(ring, "ring", (M, R, 2, V)); _chk(count, "count", (M,), dtype=torch.int32)
    for name, t in (("slot", slot), ("reset", reset), ("out_index", out_index)):
        _chk(t, name, (n,), dtype=torch.int32)
    _chk_host_i32(slot_host, "slot_host", n)
    _chk(center, "center", (34,), dtype=torch.float64, optional=True); _chk(scale, "scale", (34,), dtype=torch.float64, optional=True)
    width, height = (0.0, 0.0) if vid_res is None else (float(vid_res[0]), float(vid_res[1]))
    x_out = torch.empty(K * m, 2, T, V, device=raw.device, dtype=torch.float32) if m > 0 else None
    call("coskad_stream_push_f32", raw, slot, slot_host, reset, out_index, center, scale, width, height, flags, mats, ring, count, x_out,
         n, m, M, K, T, V, step, _stream())
    return x_out


def stream_frames(scores, slot, slot_host, clip_index, count, wscore, clip, T, step):
    """The scores [K m] of a push's windows into the tracks' score rings; -> frame_mean [K, m] f64, the row of every ready track that
    became final (`coskad_stream_frames_f64`).  clip [K, clip_frames] f64 or None: folded at clip_index [m] by a 64-bit atomic max."""
    if scores.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"scores: expected float32 or float64, got {scores.dtype}")
    M, K, R = wscore.shape
    m = slot.numel()
    _chk(scores, "scores", dtype=scores.dtype); _chk(slot, "slot", (m,), dtype=torch.int32); _chk(count, "count", (M,), dtype=torch.int32)
    _chk(wscore, "wscore", (M, K, stream_rows(T, step)), dtype=torch.float64)
    _chk_host_i32(slot_host, "slot_host", m)
    if scores.numel() != K * m:
        raise ValueError(f"scores: expected {K} x {m} values, got {scores.numel()}")
    _chk(clip, "clip", dtype=torch.float64, optional=True)
    if clip is not None:
        _chk(clip_index, "clip_index", (m,), dtype=torch.int32)
    out = torch.empty(K, m, device=scores.device, dtype=torch.float64)
    call("coskad_stream_frames_f64", scores, int(scores.dtype == torch.float64), slot, slot_host, clip_index if clip is not None else None,
         count, wscore, out, clip, clip.shape[1] if clip is not None else 0, m, M, K, T, step, _stream())
    return out


def stream_close(row_slot, row_slot_host, row_index, clip_index, count, wscore, clip, T, step):
    """The trailing rows of closed tracks, final with the windows that exist (`coskad_stream_close_f64`): row_slot / row_index [rows]
    int32 -> frame_mean [K, rows] f64, folded into clip like `stream_frames`."""
    M, K, R = wscore.shape
    rows = row_slot.numel()
    _chk(row_slot, "row_slot", (rows,), dtype=torch.int32); _chk(row_index, "row_index", (rows,), dtype=torch.int32)
    _chk(count, "count", (M,), dtype=torch.int32); _chk(wscore, "wscore", (M, K, stream_rows(T, step)), dtype=torch.float64)
    _chk_host_i32(row_slot_host, "row_slot_host", rows)
    _chk(clip, "clip", dtype=torch.float64, optional=True)
    if clip is not None:
        _chk(clip_index, "clip_index", (rows,), dtype=torch.int32)
    out = torch.empty(K, rows, device=wscore.device, dtype=torch.float64)
    call("coskad_stream_close_f64", row_slot, row_slot_host, row_index, clip_index if clip is not None else None, count, wscore, out, clip,
         clip.shape[1] if clip is not None else 0, rows, M, K, T, step, _stream())
    return out


def stream_push_cams(raw, slot, slot_host, reset, out_index, center, scale, res, res_host, flags, mats, ring, count, m, T, V, step):
    """`stream_push` for the detections of several cameras in one launch (`coskad_stream_push_cams_f32`): res [n, 2] f32 on the device =
    (width, height) of each detection's video, res_host the host's copy; both None with STREAM_NORMALISED.  -> x_out [K m, 2, T, V]
    (None at m = 0)."""
    n, M, K = raw.shape[0], count.numel(), mats.shape[0]
    R = stream_rows(T, step)
    _chk(raw, "raw", (n, 34)); _chk(mats, "mats", (K, 3, 3)); _chk(ring, "ring", (M, R, 2, V)); _chk(count, "count", (M,), dtype=torch.int32)
    for name, t in (("slot", slot), ("reset", reset), ("out_index", out_index)):
        _chk(t, name, (n,), dtype=torch.int32)
    _chk_host_i32(slot_host, "slot_host", n)
    _chk(center, "center", (34,), dtype=torch.float64, optional=True); _chk(scale, "scale", (34,), dtype=torch.float64, optional=True)
    if res is not None or not flags & STREAM_NORMALISED:
        _chk(res, "res", (n, 2))
        if res_host is None or res_host.is_cuda or res_host.dtype != torch.float32 or not res_host.is_contiguous() or res_host.numel() != 2 * n:
            raise ValueError(f"res_host: expected {2 * n} contiguous float32 values on the host")
    x_out = torch.empty(K * m, 2, T, V, device=raw.device, dtype=torch.float32) if m > 0 else None
    call("coskad_stream_push_cams_f32", raw, slot, slot_host, reset, out_index, center, scale, res, res_host, flags, mats, ring, count,
         x_out, n, m, M, K, T, V, step, _stream())
    return x_out


def stream_smooth(clip, items, items_host, taps):
    """Fixed-lag smoothing over the flat clip buffer (`coskad_stream_smooth_f64`): clip [K, F] f64, items [n_items, 3] int32 on the
    device = (segment offset, segment length, output index), items_host the host's copy, taps = gaussian_taps().
    -> (per_t [K, n_items], mean over the transformations [n_items]), float64."""
    _chk(clip, "clip", dtype=torch.float64); _chk(taps, "taps", dtype=torch.float64)
    if clip.dim() != 2:
        raise ValueError(f"clip: expected [K, F], got {tuple(clip.shape)}")
    K, F = clip.shape
    n = items.shape[0]
    _chk(items, "items", (n, 3), dtype=torch.int32)
    _chk_host_i32(items_host, "items_host", 3 * n)
    per_t = torch.empty(K, n, device=clip.device, dtype=torch.float64)
    mean = torch.empty(n, device=clip.device, dtype=torch.float64)
    call("coskad_stream_smooth_f64", clip, items, items_host, taps, taps.numel(), per_t, mean, n, K, F, _stream())
    return per_t, mean


def stream_maps_state_bytes(M: int, K: int, T: int, V: int, step: int) -> int:
    """Host arithmetic of `coskad_stream_maps_state_bytes`: fp64 sums [M, K, R, V], then int32 counts [M, K, R] rounded up to 8 bytes;
    0 for sizes the maps entries refuse.  tests/test_stream_maps_host.py holds the two in agreement."""
    if M <= 0 or K <= 0 or step <= 0 or not stream_ok(T, V) or stream_rows(T, step) > (2 ** 31 - 1) // 36:
        return 0
    rows = M * K * stream_rows(T, step)
    return rows * V * 8 + (rows * 4 + 7) // 8 * 8


def stream_maps_state(M: int, K: int, T: int, V: int, step: int, device) -> Tensor:
    """The per-track map state of `stream_maps`, as float64 words (the counts live in its tail); needs no clearing between tracks."""
    nbytes = stream_maps_state_bytes(M, K, T, V, step)
    if nbytes == 0:
        raise ValueError(f"stream_maps_state: unsupported (max_tracks={M}, K={K}, n_frames={T}, n_joints={V}, step={step})")
    return torch.zeros(nbytes // 8, device=device, dtype=torch.float64)


def stream_maps(maps, slot, slot_host, count, state, K, T, V, step):
    """The window maps [K m, T, V] f32 of a push's windows into the tracks' running sums; -> frame_map [K, m, V] f64, the map of the row
    of every ready track that became final (`coskad_stream_maps_f64`): the mean over its covering windows in ascending start, NaN where
    the track has no window.  After `stream_frames` of the same push, on every push that hands the track a window."""
    M, m = count.numel(), slot.numel()
    _chk(maps, "maps", (K * m, T, V)); _chk(slot, "slot", (m,), dtype=torch.int32); _chk(count, "count", (M,), dtype=torch.int32)
    _chk(state, "state", dtype=torch.float64)
    _chk_host_i32(slot_host, "slot_host", m)
    out = torch.empty(K, m, V, device=maps.device, dtype=torch.float64)
    call("coskad_stream_maps_f64", maps, slot, slot_host, count, state, _bytes(state), out, m, M, K, T, V, step, _stream())
    return out


def stream_maps_close(row_slot, row_slot_host, row_index, count, state, K, T, V, step):
    """The maps of the trailing rows of closed tracks, final with the windows that exist (`coskad_stream_maps_close_f64`): row_slot /
    row_index [rows] int32 -> frame_map [K, rows, V] f64; NaN for a track that never filled a window."""
    M, rows = count.numel(), row_slot.numel()
    _chk(row_slot, "row_slot", (rows,), dtype=torch.int32); _chk(row_index, "row_index", (rows,), dtype=torch.int32)
    _chk(count, "count", (M,), dtype=torch.int32); _chk(state, "state", dtype=torch.float64)
    _chk_host_i32(row_slot_host, "row_slot_host", rows)
    out = torch.empty(K, rows, V, device=state.device, dtype=torch.float64)
    call("coskad_stream_maps_close_f64", row_slot, row_slot_host, row_index, count, state, _bytes(state), out, rows, M, K, T, V, step,
         _stream())
    return out
