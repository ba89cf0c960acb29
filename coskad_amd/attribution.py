"""Joint-level anomaly attribution of the one-class encoders: the gradient of a window's own score with respect to its input
skeleton.

The eval-mode layer with folded BatchNorm, U = Wz gcn(X) + Wx X + b with X = PReLU(in), has no batch coupling, so its adjoint
dIn = PReLU'(in) (.) (gcn^T(Wz^T dU) + Wx^T dU) is one kernel per layer with one clip per workgroup (csrc/eval_layer_adj.hip).  The
chain of `window_attribution`:
  1. an unfused eval forward that keeps every layer's pre-activation U_1 .. U_n (ops.layer_apply with the eval-mode folded weights
     of engine.eval_fold; neither the first-pair kernel nor the one-kernel encoder, which keep them on chip);
  2. ops.btlnk_fwd;
  3. the head with need_grad and upstream = B: the heads differentiate a MEAN over the batch, B turns that into each window's own
     score (Euclidean: d mean_j (z - c)^2; Poincare: d dist(c, z_h); Mahalanobis: d sqrt(d^T VI d));
  4. ops.btlnk_bwd for dU_n (its dW / db outputs go to scratch);
  5. one ops.layer_input_grad per layer, last to first.
Everything outside the supported set raises ValueError naming the reason; nothing falls back.

The decoder models' counterpart: `window_latent_attribution` runs the same chain on the autoencoder's encoder for the
latent term of its score, and `dataset_error_maps` writes the per-joint reconstruction-error maps of `lit.window_error_map` -- no
gradient: the map is the decomposition of the reconstruction term that the decoder-tail kernel forms beside the score.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import engine, ops

Tensor = torch.Tensor


def unsupported_reason(lit) -> Optional[str]:
    """Why `lit.window_attribution` does not take this wrapper in its current mode (host arithmetic, no device), or None."""
    model = getattr(lit, "model", None)
    if model is None or hasattr(model, "decoder") or hasattr(model, "rev_btlnk") or not hasattr(model, "btlnk"):
        return "autoencoder / VAE wrappers have a decoder: their natural map is the per-joint reconstruction error, not an input gradient"
    return encoder_unsupported_reason(model)


def encoder_unsupported_reason(model) -> Optional[str]:
    """Why the adjoint chain does not run through this model's encoder and bottleneck in its current mode (host arithmetic), or None:
    the encoder-side half of `unsupported_reason`, which LitAutoEncoder.window_latent_attribution asks on its own."""
    from .models.common.components import Encoder
    if model.training:
        return "train mode: BatchNorm couples the batch; call .eval() (the adjoint is that of the layers with folded running statistics)"
    if not isinstance(model.encoder, Encoder):
        return f"encoder_type {model.encoder_type!r}: plain-GCN encoders have no folded-layer adjoint (STS_GCN only)"
    if model.projector != 'linear' or not isinstance(model.btlnk, nn.Linear):
        return f"projector {model.projector!r}: only the `linear` projector has a bottleneck backward here (mlp is out of scope)"
    if not 0 < model.latent_dim <= ops.BTLNK_LMAX:
        return f"latent_dim {model.latent_dim}: the bottleneck backward takes 1 .. {ops.BTLNK_LMAX}"
    T, V = model.n_frames, model.n_joints
    if V not in ops.INPUT_GRAD_JOINTS:
        return f"n_joints V = {V}: the adjoint kernel is built for V in {list(ops.INPUT_GRAD_JOINTS)} (14 / 18 are out of scope)"
    if T not in ops.INPUT_GRAD_FRAMES:
        return f"n_frames T = {T}: the adjoint kernel is built for T in {list(ops.INPUT_GRAD_FRAMES)}"
    for i, m in enumerate(model.encoder.model):
        if m.dropout > 0:
            return f"layer {i} has dropout {m.dropout}: layers with dropout run the composed path, which has no folded form"
        if not ops.layer_input_grad_ok(T, V, m.in_channels, m.out_channels):
            return (f"layer {i} ({m.in_channels} -> {m.out_channels}) is wide: the adjoint kernel takes "
                    f"{list(ops.INPUT_GRAD_CIN)} -> {list(ops.INPUT_GRAD_COUT)} channels")
        bns = [m.tcn[1]] + ([] if isinstance(m.residual, nn.Identity) else [m.residual[1]])
        if not all(bn.track_running_stats and bn.running_mean is not None for bn in bns):
            return f"layer {i}: BatchNorm without running statistics normalises with batch statistics in eval mode too"
    return None


def _first_layer_window(x: Tensor, L: engine.LayerTensors, wfold: Tensor, bias: Tensor) -> Tensor:
    """The network-input layer (2 -> Co) at a window length other than 12, where ops.layer_apply has no kernel for two input
    channels: the mixing kernel, then [Wz; Wx]^T [Z; x] + b on the strided GEMM -- the same folded weights."""
    B, Ci, T, V = x.shape
    Co = L.Co
    zx = torch.cat([ops.gcn(x, L.A, L.T), x], 1).view(B, 2 * Ci, T * V)
    u = ops.gemm(wfold[:, :Co].t(), zx, bias=bias[:Co], bias_mode=1, bias_mod=Co)
    return u.view(B, Co, T, V)


def eval_preactivations(x: Tensor, layers: List[engine.LayerTensors]) -> Tuple[List[Tensor], List[Tuple[Tensor, Tensor]]]:
    """-> ([U_1 .. U_n], [(wfold, bias)]): every layer's pre-activation of the eval-mode forward, one launch per layer."""
    B, C, T, V = x.shape
    us, folds = [], []
    h, slope = x, None
    for L in layers:
        wfold, bias = engine.eval_fold(L)
        if slope is None and T != 12 and not ops.layer_apply_window_ok(T, V, L.Ci, L.Co):
            u = _first_layer_window(h, L, wfold, bias)
        else:
            u = ops.layer_apply(h, L.A, L.T, wfold, bias, L.Co, in_slope=slope)
        us.append(u)
        folds.append((wfold, bias))
        h, slope = u, L.slope
    return us, folds


def head_score_grad(lit, z: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (score [B], dz [B, L] = d score_n / d z_n) from the wrapper's head: upstream = B undoes the heads' mean over the batch"""
    B = z.shape[0]
    c = lit.model.c
    if lit.hyperbolic:
        _, dz, _, score = ops.poincare_head(z, c, need_grad=True, need_score=True, upstream=float(B))
    elif lit.distance == 'mahalanobis':
        _, dz, score = ops.mahalanobis_head(z, c, lit.model.inv_cov_matrix, need_grad=True, need_score=True, upstream=float(B))
    else:
        _, dz, score = ops.mse_head(z, c, need_grad=True, need_score=True, upstream=float(B))
    return score, dz


def dataset_attribution(lit, loader, outputs, directory: str) -> None:
    """The attribution maps of a whole test pass as per-clip files (eval_COSKAD.py --attribution-dir): `loader()` yields the batches
    [x, trans, meta, frames] that `outputs` (Trainer.predict's list) came from.  Every window's map attr [T, V] is held on the device
    -- N T V floats for N windows -- then turned into person-frame maps by eval_utils.attribution_frames_device on the scoring plan's
    window table and written by eval_utils.save_attribution."""
    from .utils import eval_utils
    why = unsupported_reason(lit)
    if why is not None:
        raise ValueError(f"window_attribution: {why}")
    dev = lit.model.c.device
    attr = torch.cat([window_attribution(lit, b[0])[2] for b in loader()], 0)
    trans, meta, frames = (torch.cat([o[i] for o in outputs], 0) for i in (1, 2, 3))
    if attr.shape[0] != frames.shape[0]:
        raise ValueError(f"dataset_attribution: {attr.shape[0]} maps for a window table of {frames.shape[0]} rows")
    num_transform = max(1, int(getattr(lit.args, "dataset_num_transform", 1)))
    plan = getattr(lit, "_score_plan", None)
    if plan is None or plan.win_ptr.device != attr.device or plan.num_transform != num_transform or not plan.matches(trans, meta, frames):
        plan = eval_utils.ScorePlan(trans, meta, frames, lit._load_gts(), num_transform, device=dev)
    eval_utils.save_attribution(directory, eval_utils.attribution_frames_device(attr, frames, plan), plan)


def window_attribution(lit, x: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (score [B], grad [B, C, T, V] = d score_n / d x_n, attr [B, T, V] = sum_c x * grad) for a LitEncoder in eval mode."""
    why = unsupported_reason(lit)
    if why is not None:
        raise ValueError(f"window_attribution: {why}")
    return _input_gradient(lit.model, x, lambda z: head_score_grad(lit, z), "window_attribution")


def window_latent_attribution(lit, x: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (hyp [B], grad [B, C, T, V] = d hyp_n / d x_n, attr [B, T, V] = sum_c x * grad) for a LitAutoEncoder in eval mode: the chain
    of `window_attribution` on the autoencoder's encoder and bottleneck with the Euclidean head on its centre, hyp = mean_j (z - c)^2
    -- the latent term of the autoencoder's score.  The decoder does not run."""
    model = getattr(lit, "model", None)
    if model is None or not hasattr(model, "decoder") or not hasattr(model, "btlnk") or hasattr(model, "mean_vector"):
        raise ValueError("window_latent_attribution: the autoencoder wrapper only (a one-class encoder has `window_attribution`; the "
                         "VAE's score is the cosine of a sampled latent)")
    why = encoder_unsupported_reason(model)
    if why is not None:
        raise ValueError(f"window_latent_attribution: {why}")

    def head(z):
        _, dz, score = ops.mse_head(z, model.c, need_grad=True, need_score=True, upstream=float(z.shape[0]))
        return score, dz
    return _input_gradient(model, x, head, "window_latent_attribution")


def dataset_error_maps(lit, loader, outputs, directory: str) -> None:
    """The reconstruction-error maps of a whole test pass as per-clip files (eval_COSKAD.py --error-map-dir): `dataset_attribution`'s
    flow with `lit.window_error_map` -- every window's map [T, V] is held on the device (N T V floats for N windows), turned into
    person-frame maps by eval_utils.attribution_frames_device on the scoring plan's window table (the mean over the covering windows)
    and written by eval_utils.save_attribution as `<scene>_<clip>_error_map.npy` (mean over the transformations, NaN where the person
    is absent) and `<scene>_<clip>_persons.npy`.  The wrapper's ValueError for a wrapper without a decoder or without a reconstruction
    term in its score."""
    from .utils import eval_utils
    maps = [lit.window_error_map(b[0])[1] for b in loader()]
    if not maps:
        raise ValueError("dataset_error_maps: the loader yields no batch")
    emap = torch.cat(maps, 0)
    trans, meta, frames = (torch.cat([o[i] for o in outputs], 0) for i in (1, 2, 3))
    if emap.shape[0] != frames.shape[0]:
        raise ValueError(f"dataset_error_maps: {emap.shape[0]} maps for a window table of {frames.shape[0]} rows")
    num_transform = max(1, int(getattr(lit.args, "dataset_num_transform", 1)))
    plan = getattr(lit, "_score_plan", None)
    if plan is None or plan.win_ptr.device != emap.device or plan.num_transform != num_transform or not plan.matches(trans, meta, frames):
        plan = eval_utils.ScorePlan(trans, meta, frames, lit._load_gts(), num_transform, device=emap.device)
    eval_utils.save_attribution(directory, eval_utils.attribution_frames_device(emap, frames, plan), plan, suffix="error_map")


def _input_gradient(model, x: Tensor, head, what: str) -> Tuple[Tensor, Tensor, Tensor]:
    """the chain of the module's docstring through `model`'s encoder and bottleneck; `head`: z -> (score [B], dz [B, L])"""
    from .models.graph_layers.stsgcn import layer_tensors
    if x.dim() != 4 or tuple(x.shape[1:]) != (model.input_dim, model.n_frames, model.n_joints):
        raise ValueError(f"{what}: expected x [B, {model.input_dim}, {model.n_frames}, {model.n_joints}], got {tuple(x.shape)}")
    if x.shape[0] < 1:
        raise ValueError(f"{what}: empty batch")
    with torch.no_grad():
        x = x.to(model.c.device, torch.float32).contiguous()
        B = x.shape[0]
        layers = [layer_tensors(m) for m in model.encoder.model]
        us, folds = eval_preactivations(x, layers)
        W, top = model.btlnk.weight.contiguous(), layers[-1].slope
        z = ops.btlnk_fwd(us[-1], W, model.btlnk.bias, top, ws=model._ws)
        score, dz = head(z)
        K, Lz = W.shape[1], W.shape[0]
        # the parameter gradients the bottleneck backward also forms are scratch here
        dW = torch.empty_like(W)
        db = torch.empty(Lz, device=W.device, dtype=torch.float32) if model.btlnk.bias is not None else None
        buf = torch.empty(ops.btlnk_bwd_ws_bytes(B, K, Lz), dtype=torch.uint8, device=W.device)
        g = ops.btlnk_bwd(us[-1], W, dz, top, dW, db, None, buf)
        for i in range(len(layers) - 1, -1, -1):
            L = layers[i]
            x_in, slope = (us[i - 1], layers[i - 1].slope) if i > 0 else (x, None)
            g = ops.layer_input_grad(g, x_in, L.A, L.T, folds[i][0], L.Co, in_slope=slope)
        attr = (x * g).sum(1)
    return score, g, attr
