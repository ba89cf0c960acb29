"""Lightning-style wrapper of the one-class STSE training (mirror of the reference's
models/euclidean_encoder_staticCenter.py, models/euclidean_encoder_dynamicCenter.py and
models/hyperbolic_encoder.py `LitEncoder`, which cannot be imported from the snapshot -- SURVEY fact 1 --
and a minimal `Trainer` replacing pytorch_lightning, which is not installed).

Same hooks and config keys (flat yaml -> argparse.Namespace): `forward(x: list[4])`, `setup(stage)`,
`training_step`, `on_train_epoch_end`, `validation_step`, `validation_epoch_end`, `configure_optimizers`,
`post_processing`.  Differences, all deliberate:
  * the optimisation step is the fused HIP sequence of coskad_amd.trainer.STSETrainStep (forward, loss,
    backward, L2 reg, Adam in one call), so `training_step` has already stepped when it returns the loss;
  * centre statistics are device-side running sums (and all-reduced over ranks) instead of python lists /
    torch.cat of every latent (hyperbolic_encoder.py:148-153);
  * post_processing is the vectorised scoring of coskad_amd.utils.eval_utils.
Parity of these wrappers against the reference is unpinned (no importable reference, no recorded numbers).
"""
from __future__ import annotations

import os
from argparse import Namespace
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, parallel
from .models.sts.ae import STSE
from .trainer import STSETrainStep, make_train_step
from .utils import eval_utils


def _joints(args) -> int:
    if getattr(args, "dataset_headless", False):
        return 14
    if getattr(args, "dataset_kp18_format", False):
        return 18
    return 17


def step_knobs(args) -> Dict:
    """Lightning's Trainer arguments that act on the optimisation step, under Lightning's names (the reference hands every yaml
    key to pl.Trainer.from_argparse_args, train_COSKAD.py:75-78) -> the step classes' keywords"""
    return {"grad_clip_val": getattr(args, "gradient_clip_val", None) or 0.0,
            "grad_clip_algorithm": getattr(args, "gradient_clip_algorithm", None) or "norm",
            "accumulate": int(getattr(args, "accumulate_grad_batches", None) or 1)}


# wrapper state that is no buffer of the model and that a resumed run needs (Trainer.fit(ckpt_path=...))
_RESUME_ATTRS = ("_epoch", "_temp", "n_samples", "_reg_last", "warmup_counter")


class LitEncoder(nn.Module):
    _reg_last = None      # the regulariser's value at the last logging step (training_step reuses it in between)
    n_samples = None

    # ---- what a checkpoint carries beside the model's state_dict, and its way back (Trainer.fit(ckpt_path=...)) ------------
    def optimizer_state(self) -> Dict:
        return self._engine.state_dict()

    def load_optimizer_state(self, sd: Dict) -> None:
        self._engine.load_state_dict(sd)

    def resume_state(self) -> Dict:
        return {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v)
                for k, v in ((k, getattr(self, k)) for k in _RESUME_ATTRS if hasattr(self, k))}

    def load_resume_state(self, state: Dict) -> None:
        dev = next(self.model.parameters()).device
        for k, v in state.items():
            setattr(self, k, v.to(dev) if torch.is_tensor(v) else v)

    def flush_gradients(self) -> None:
        """the update of a pending accumulation group (Lightning steps on the last batch of an epoch whatever its index)"""
        self._engine.flush()

    def _log_grad_norm(self, step, batch_idx: int) -> None:
        """`grad_norm`, the unclipped norm of the last update, when clipping by norm -- the only host read of it"""
        if batch_idx % 20 == 0 and step.clip_val > 0 and step.clip_mode == 'norm':
            self.log("grad_norm", step.last_grad_norm)

    def __init__(self, args: Namespace, hyperbolic: Optional[bool] = None) -> None:
        super().__init__()
        self.args = args
        self.hparams = Namespace(args=args)                  # save_hyperparameters()
        self.hyperbolic = bool(getattr(args, "hyperbolic", False) if hyperbolic is None else hyperbolic)
        self.static_center = bool(getattr(args, "static_center", False))
        self.distance = str(getattr(args, "distance", "euclidean")).lower()   # staticCenter.py:66,84: 'mahalanobis' option
        channels = list(getattr(args, "channels", [32, 16, 32]))
        self.eps = float(getattr(args, "center_tolerance", 1e-3))
        self.model = STSE(c_in=args.num_coords, h_dim=args.h_dim, latent_dim=args.latent_dim,
                          n_frames=args.dataset_seg_len, dropout=args.dropout, n_joints=_joints(args),
                          channels=channels, projector=getattr(args, "projector", "linear"),
                          encoder_type=getattr(args, "encoder_type", "STS_GCN"), distance=self.distance)
        self.learning_rate = args.opt_lr
        self.batch_size = getattr(args, "dataset_batch_size", 2048)
        self.logged: Dict[str, float] = {}
        self._engine: Optional[STSETrainStep] = None
        self._epoch = 0
        self._temp = None
        self.gts: Optional[Dict[Tuple[int, int], np.ndarray]] = None   # frame masks; else read from args.gt_path

    # ---- inference ---------------------------------------------------------------------
    def forward(self, x):
        tensor_data, transformation_idx, metadata, actual_frames = x[0], x[1], x[2], x[3]
        hidden_out = self.model(tensor_data)
        return hidden_out, transformation_idx, metadata, actual_frames

    def log(self, name: str, value) -> None:
        self.logged[name] = float(value)

    # ---- centre initialisation (staticCenter.py:95-130, dynamicCenter.py:76-102, hyperbolic_encoder.py:85-135)
    def setup(self, stage: str = None, train_loader: Optional[Callable[[], Iterable]] = None, resume: bool = False) -> None:
        """resume: build the step only; the centre, its covariance and the wrapper's own state come from the checkpoint"""
        if stage != "fit":
            return
        maha = self.distance == 'mahalanobis' and not self.hyperbolic
        if not resume:
            self._init_center(train_loader, maha)
        self._build_step(maha)

    def _init_center(self, train_loader, maha: bool) -> None:
        dev = next(self.model.parameters()).device
        L = self.model.latent_dim
        acc = torch.zeros(ops.head_slots(L), device=dev)
        gram = torch.zeros(L, L, device=dev) if maha else None
        eye = torch.eye(L, device=dev) if maha else None
        self.model.eval()
        with torch.no_grad():
            for batch in train_loader():
                z = self.model(batch[0].to(dev).contiguous())
                if self.hyperbolic:
                    ops.poincare_head(z, None, need_grad=False, acc=acc)
                elif maha:                                  # centre sums + second moments in one pass
                    ops.mahalanobis_head(z, self.model.c, eye, need_grad=False, acc=acc, gram=gram)
                else:
                    ops.mse_head(z, self.model.c, need_grad=False, acc=acc)
        parallel.allreduce_sum_(acc)
        if maha:
            parallel.allreduce_sum_(gram)
        self.n_samples = float(acc[ops.head_count_slot(L)]) if not self.hyperbolic else None
        if self.hyperbolic:
            c = ops.midpoint_finalize(acc, L)
            assert bool((c < 1).all()), f"center is out of the ball\nc = {c}"        # hyperbolic_encoder.py:123
            self.model.c.copy_(c)
        elif self.static_center:
            self.model.c.copy_(ops.center_finalize(acc, self.eps, L))                 # staticCenter.py:118-123
        else:
            # dynamicCenter.py:96-100: the initial centre is stored but model.c stays 0 during the first epoch
            self._temp = ops.center_finalize(acc, 0.0, L)
        if maha:                                            # staticCenter.py:124-127,133-142
            from .trainer import inv_cov_from_moments
            mu = self.model.c if self.static_center else self._temp
            self.model.inv_cov_matrix.copy_(inv_cov_from_moments(gram, acc, mu, L))

    def _build_step(self, maha: bool) -> None:
        self.model.train()
        # `sync_batchnorm` (not a key of the reference's yamls, whose DDP keeps per-rank BatchNorm statistics): optional SyncBN
        extra = {"sync_bn": True} if bool(getattr(self.args, "sync_batchnorm", False)) else {}
        # `flat_plain_gcn` (not a key of the reference's yamls either): the Learnable_GCN / Static_GCN encoders train on the flat step
        # with the fused layer kernels unless the yaml says `flat_plain_gcn: false` (then: the autograd step)
        extra["flat_plain_gcn"] = bool(getattr(self.args, "flat_plain_gcn", True))
        # `fused_window` (not a key of the reference's yamls either): encoders of `dataset_seg_len` 8 / 16 / 24 train on the stored-Z layer
        # kernels where those are built unless the yaml says `fused_window: false` (then: the composed path)
        extra["fused_window"] = bool(getattr(self.args, "fused_window", True))
        self._engine = make_train_step(self.model, lr=self.learning_rate, alpha=float(getattr(self.args, "alpha", 0.0)),
                                     head="poincare" if self.hyperbolic else ("mahalanobis" if maha else "euclidean"), **extra,
                                     **step_knobs(self.args))
        self._epoch = 0

    # ---- one optimisation step -----------------------------------------------------------
    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        dev = self.model.c.device
        stats = self._engine.step(batch[0].to(dev, non_blocking=True).contiguous())
        # the reference returns head + alpha * reg (staticCenter.py:180-189); the regulariser is evaluated when it is logged
        # (two launches) and that value is reused for the steps in between: at alpha ~ 1e-6 it moves in the 7th digit per step
        if batch_idx % 20 == 0 or self._reg_last is None: # log_every_n_steps=20 (train_COSKAD.py:76)
            self._reg_last = self._engine.reg_loss().reshape(())
        loss = stats[0] + self._engine.alpha * self._reg_last
        if batch_idx % 20 == 0:
            name = "poincare_loss" if self.hyperbolic else "hypersphere_loss"
            self.log(name, stats[0]); self.log("regularization", self._reg_last)
            self.log("loss", float(loss))
        self._log_grad_norm(self._engine, batch_idx)
        return loss

    def on_train_epoch_end(self) -> None:
        eng = self._engine
        if eng.head == 'mahalanobis':                      # staticCenter.py:146-147 (before the centre update)
            eng.refresh_inv_cov(self.model.c)
        if self.hyperbolic:
            if not self.static_center:                     # hyperbolic_encoder.py:175-183
                c = eng.refresh_center()
                self.log("center/eucl", torch.linalg.norm(c))
            else:
                eng.center_acc.zero_()
        elif self.static_center:
            eng.center_acc.zero_()
        else:                                              # dynamicCenter.py:125-142
            if self._epoch == 0:
                parallel.allreduce_sum_(eng.center_acc)
                self.model.c.copy_(self._temp)
                eng.center_acc.zero_()
            else:
                eng.refresh_center(eps=self.eps)
        self._epoch += 1

    training_epoch_end = on_train_epoch_end

    def configure_optimizers(self) -> Dict:
        """Adam(lr=opt_lr) (+ ReduceLROnPlateau(mode='max', factor=0.2, min_lr=1e-6) on validation_auc when
        args.validation); the HIP engine owns the Adam state, the Trainer applies the plateau rule."""
        return {"optimizer": "adam", "lr": self.learning_rate,
                "lr_scheduler": {"name": "ReduceLROnPlateau", "mode": "max", "factor": 0.2,
                                 "patience": 2 if not self.static_center and not self.hyperbolic else 100,
                                 "min_lr": 1e-6},
                "monitor": "validation_auc"}

    # ---- validation / scoring --------------------------------------------------------------
    def validation_step(self, batch, batch_idx: int = 0):
        dev = next(self.model.parameters()).device
        with torch.no_grad():
            return self.forward([batch[0].to(dev).contiguous(), batch[1], batch[2], batch[3]])

    predict_step = validation_step

    def validation_epoch_end(self, outputs: List) -> float:
        hidden = torch.cat([o[0] for o in outputs], 0)
        trans = torch.cat([o[1] for o in outputs], 0)
        meta = torch.cat([o[2] for o in outputs], 0)
        frames = torch.cat([o[3] for o in outputs], 0)
        return self.post_processing(hidden, trans, meta, frames)

    def window_scores(self, hidden: torch.Tensor) -> torch.Tensor:
        """per-window anomaly score on the device (eval_utils.py:63-67)."""
        if self.hyperbolic:
            _, _, _, score = ops.poincare_head(hidden.contiguous(), self.model.c, need_grad=False, need_score=True)
        elif self.distance == 'mahalanobis':               # eval_utils.py:41-47
            _, _, score = ops.mahalanobis_head(hidden.contiguous(), self.model.c, self.model.inv_cov_matrix,
                                               need_grad=False, need_score=True)
        else:
            _, _, score = ops.mse_head(hidden.contiguous(), self.model.c, need_grad=False, need_score=True)
        return score

    def window_attribution(self, x: torch.Tensor):
        """-> (score [B], grad [B, C, T, V], attr [B, T, V]) of a batch of windows, eval mode: each window's own score (what
        `window_scores` gives for the same batch), its gradient with respect to the input skeleton and gradient x input summed over
        the coordinates -- which person-frame-joint carries the score; a missing joint (an exact 0 in x) gets 0.  The adjoint of the
        folded eval layers on csrc/eval_layer_adj.hip (coskad_amd/attribution.py).  ValueError naming the reason outside
        the supported set (train mode, mlp projector, plain-GCN encoders, V = 14 / 18, wide layers, dropout)."""
        from . import attribution
        return attribution.window_attribution(self, x)

    def window_error_map(self, x: torch.Tensor):
        raise ValueError(f"window_error_map: {type(self).__name__} has no decoder, so there is no reconstruction to take the error of; "
                         "`window_attribution` is the map of a one-class encoder")

    def _load_gts(self) -> Dict[Tuple[int, int], np.ndarray]:
        if self.gts is not None:
            return self.gts
        out = {}
        for fn in sorted(os.listdir(self.args.gt_path)):
            if fn.endswith(".npy"):
                sc, cl = int(fn.split("_")[0]), int(fn.split("_")[1].split(".")[0])
                out[(sc, cl)] = np.load(os.path.join(self.args.gt_path, fn))
        return out

    def _load_hr_masks(self) -> Optional[Dict[Tuple[int, int], np.ndarray]]:
        """Human-related frame subsets (eval_COSKAD.py:86-97, utils/model_utils.py:149-161): `use_hr: True` +
        `hr_mask_path` (a glob of `<scene>_<clip>.npy` boolean masks; the reference hard-codes its own disk path), or
        masks assigned to `self.hr_masks`."""
        if getattr(self, "hr_masks", None) is not None:
            return self.hr_masks
        if getattr(self.args, "use_hr", False) and getattr(self.args, "hr_mask_path", None):
            return eval_utils.hr_masks_from_dir(self.args.hr_mask_path)
        return None

    def post_processing(self, hidden_out, trans, meta, frames) -> float:
        return self._score_windows(self.window_scores(hidden_out), trans, meta, frames)

    def _score_windows(self, scores, trans, meta, frames) -> float:
        """window scores -> frames -> persons -> smoothing -> transformations -> AUC (eval_COSKAD.py:140-253)."""
        num_transform = max(1, int(getattr(self.args, "dataset_num_transform", 1)))
        gts, pad_size, hr_masks = self._load_gts(), int(getattr(self.args, "pad_size", -1)), self._load_hr_masks()
        # `device_scoring` (not a key of the reference's yamls either): scores that live on the GPU are turned into the frame-level AUC
        # by the scoring kernels on a plan of the window table, built at the first call and reused while the table is the same one,
        # unless the yaml says `device_scoring: false` (then: eval_utils.score_dataset, as for scores on the host)
        # `eval_report` (no key of the reference's yamls; off unless set): also the reference's per-clip AUCs, per-transformation AUCs
        # and ROC thresholds, on the same route as the scoring, kept as `self.last_report`
        report = bool(getattr(self.args, "eval_report", False))
        if bool(getattr(self.args, "device_scoring", True)) and torch.as_tensor(scores).is_cuda:
            plan = getattr(self, "_score_plan", None)
            if plan is None or plan.win_ptr.device != scores.device or not plan.same_setting(gts, num_transform, pad_size, hr_masks) \
                    or not plan.matches(trans, meta, frames):
                plan = eval_utils.ScorePlan(trans, meta, frames, gts, num_transform, pad_size=pad_size, hr_masks=hr_masks,
                                            device=scores.device)
                object.__setattr__(self, "_score_plan", plan)      # not a submodule, not part of the state dict
            if report:
                self.last_report, per_t_dev, gt = eval_utils.score_report_device(scores, plan)
                auc = self.last_report.auc
            else:
                auc, per_t_dev, gt = eval_utils.score_dataset_device(scores, plan)
            per_t_host = per_t_dev.cpu().numpy()                   # one device -> host copy
            per_t = {t: per_t_host[t] for t in range(num_transform)}
        else:
            auc, per_t, gt = eval_utils.score_dataset(scores, trans, meta, frames, gts, num_transform,
                                                      smoothing=int(getattr(self.args, "smoothing", 50)),
                                                      dataname=getattr(self.args, "dataset_choice", "UBnormal"),
                                                      pad_size=pad_size, hr_masks=hr_masks)
            if report:
                keys, segments = eval_utils.clip_segments(gts, hr_masks)
                self.last_report = eval_utils.score_report(per_t, gt, segments, keys)
        if report:
            defined = self.last_report.clip_auc_mean_t[~np.isnan(self.last_report.clip_auc_mean_t)]
            self.log("validation_clip_auc_mean", defined.mean() if defined.size else float("nan"))
        self.log("validation_auc", auc)
        self.last_scores = per_t
        return auc


class _AutogradLit(LitEncoder):
    """Shared machinery of the wrappers whose loss involves the decoder (autoencoder, spherical VAE): the model runs
    through its module surface (autograd nodes around the HIP kernels), torch's Adam optimises, gradients are averaged
    over ranks.  Validation outputs are per-window scores computed on the device."""

    model_cls = None

    def window_attribution(self, x: torch.Tensor):
        raise ValueError(f"window_attribution: {type(self).__name__} scores windows by reconstruction (autoencoder / VAE wrappers): the "
                         "per-joint reconstruction error is their natural map, the input gradient of a one-class score is not defined")

    def window_error_map(self, x: torch.Tensor):
        """-> (rec [B], emap [B, T, V]) of a batch of windows, eval mode: the window's mean squared reconstruction error and its exact
        decomposition over (frame, joint), emap = ((x_rec - x)^2).sum(coordinates) / (C T V), so that emap[n].sum() == rec[n] -- where
        the skeleton was reconstructed badly.  Where the model's decoder tail is on csrc/eval_tail_window.hip the map leaves the launch
        that forms rec; otherwise it is the formula on the model's reconstruction.
        The map is of the reconstruction term, UNSCALED: under LitAutoEncoder's 'rec+hyp' the score's reconstruction part is rec /
        rec_loss_weight (plus the latent term, whose map is `window_latent_attribution`).  For LitVAE it is the map of the sampled
        latent's reconstruction (under the same torch seed: forward's) and NOT a decomposition of its score, the cosine distance of
        that latent.  Missing joints (exact zeros in x) are not masked: the reference's score counts them, and masking would break
        emap.sum() == rec.  ValueError in train mode (BatchNorm would couple the batch)."""
        why = self._error_map_refusal()
        if why is not None:
            raise ValueError(f"window_error_map: {why}")
        model = self.model
        if x.dim() != 4 or tuple(x.shape[1:]) != (model.input_dim, model.n_frames, model.n_joints):
            raise ValueError(f"window_error_map: expected x [B, {model.input_dim}, {model.n_frames}, {model.n_joints}], got {tuple(x.shape)}")
        if x.shape[0] < 1:
            raise ValueError("window_error_map: empty batch")
        with torch.no_grad():
            _, rec, emap = model.reconstruction_map(x.to(model.c.device, torch.float32).contiguous())
        return rec, emap

    def _error_map_refusal(self) -> Optional[str]:
        """why `window_error_map` does not take this wrapper in its current mode (host arithmetic), or None"""
        if self.model.training:
            return ("train mode: BatchNorm couples the batch and the reconstruction is not the scored one; call .eval() "
                    "(Trainer.predict / validate do)")
        return None

    def _build(self, args: Namespace, **extra) -> None:
        nn.Module.__init__(self)
        self.args, self.hparams = args, Namespace(args=args)
        self.hyperbolic, self.static_center, self.distance = False, True, 'euclidean'
        self.eps = float(getattr(args, "center_tolerance", 1e-3))
        self.model = self.model_cls(c_in=args.num_coords, h_dim=args.h_dim, latent_dim=args.latent_dim,
                                    n_frames=args.dataset_seg_len, dropout=args.dropout, n_joints=_joints(args),
                                    channels=list(getattr(args, "channels", [32, 16, 32])), **extra)
        self.learning_rate = args.opt_lr
        self.batch_size = getattr(args, "dataset_batch_size", 2048)
        self.logged: Dict[str, float] = {}
        self.gts = None
        object.__setattr__(self, "_engine", self)   # the Trainer's plateau rule calls _engine.set_lr (not a submodule)
        self._opt = None
        self._flat = None
        self._micro = 0                    # backward passes of the pending accumulation group (autograd route)

    # the step the clip settings and the last gradient norm live on: the flat step, or this wrapper on the autograd route
    @property
    def clip_val(self) -> float:
        return self._knobs["grad_clip_val"]

    @property
    def clip_mode(self) -> str:
        return self._knobs["grad_clip_algorithm"]

    def optimizer_state(self) -> Dict:
        if self._flat is not None:
            return self._flat.state_dict()
        return dict(self._opt.state_dict(), coskad={"micro_step": self._micro})

    def load_optimizer_state(self, sd: Dict) -> None:
        if self._flat is not None:
            return self._flat.load_state_dict(sd)
        from .trainer import _load_torch_optimizer
        _load_torch_optimizer(self._opt, sd)

    def flush_gradients(self) -> None:
        if self._flat is not None:
            self._flat.flush()
        elif self._micro:
            from .trainer import _clipped_update
            _clipped_update(list(self.model.parameters()), self._opt, None, self.clip_val, self.clip_mode, self.last_grad_norm)
            self._micro = 0

    def set_lr(self, lr: float) -> None:
        if self._flat is not None:
            self._flat.set_lr(lr)
            return
        for g in self._opt.param_groups:
            g['lr'] = lr

    def _on_device(self) -> bool:
        """the model sits on the GPU: the flat step is then asked for (a model left on the host takes the autograd route)"""
        return next(self.model.parameters()).is_cuda

    def _make_optimiser(self, mode: str, **weights) -> None:
        """The flat-buffer step with the fused Adam (trainer.STSAETrainStep: no autograd around the encoder / decoder chains)
        where the model is within its kernels; torch autograd + torch.optim.Adam over the module surface otherwise."""
        from .trainer import make_decoder_step, _check_accumulate, _check_clip
        self._flat = None
        self._knobs = step_knobs(self.args)
        self._knobs["grad_clip_val"], self._knobs["grad_clip_algorithm"] = _check_clip(self._knobs["grad_clip_val"],
                                                                                       self._knobs["grad_clip_algorithm"])
        self._knobs["accumulate"] = _check_accumulate(self._knobs["accumulate"])
        self.last_grad_norm = torch.zeros(1, device=next(self.model.parameters()).device)
        # `flat_wide_latent` (not a key of the reference's yamls; default on): false keeps a model with latent_dim > 16 on the autograd route
        # `flat_gaussian_head` (likewise): false keeps the `distribution: 'normal'` head of the flat step under its local autograd graph
        if self._on_device():
            self._flat = make_decoder_step(self.model, mode, fused_window=bool(getattr(self.args, "fused_window", True)),
                                           wide_latent=bool(getattr(self.args, "flat_wide_latent", True)),
                                           gaussian_head=bool(getattr(self.args, "flat_gaussian_head", True)),
                                           lr=self.learning_rate, alpha=float(getattr(self.args, "alpha", 0.0)), **weights,
                                           **self._knobs)
        if self._flat is None:
            self._opt = torch.optim.Adam(self.model.parameters(), lr=self.learning_rate)
        if parallel.rank() == 0:           # one line of the training log: which step and which stage forms drive this model
            print("train step: " + ("torch autograd + torch.optim.Adam" if self._flat is None else
                                    f"{type(self._flat).__name__} (projector {type(self._flat.projector).__name__}, "
                                    f"latent {type(self._flat.latent).__name__}, entry {type(self._flat.entry).__name__})"), flush=True)

    def _reg_loss(self) -> torch.Tensor:
        """utils/model_utils.py:90-105 (differentiable: it is part of these wrappers' loss)."""
        ps = [p for n, p in self.model.named_parameters() if 'bias' not in n]
        return 0.5 * sum((p ** 2).sum() for p in ps) / len(ps)

    def _optimise(self, loss: torch.Tensor) -> None:
        """backward of loss / accumulate into .grad (no zero_grad inside a group); the group's last call averages the gradients over
        ranks (one flat bucket per update), clips them and steps"""
        k = self._knobs["accumulate"]
        if self._micro == 0:
            self._opt.zero_grad(set_to_none=True)
        (loss if k == 1 else loss / k).backward()
        self._micro += 1
        if self._micro == k:
            self.flush_gradients()

    def validation_step(self, batch, batch_idx: int = 0):
        dev = self.model.c.device
        with torch.no_grad():
            return self.window_scores_from_batch(batch[0].to(dev)), batch[1], batch[2], batch[3]

    predict_step = validation_step

    def validation_epoch_end(self, outputs: List) -> float:
        scores, trans, meta, frames = (torch.cat([o[i] for o in outputs], 0) for i in range(4))
        return self._score_windows(scores, trans, meta, frames)

    def on_train_epoch_end(self) -> None:
        pass

    training_epoch_end = on_train_epoch_end

    def configure_optimizers(self) -> Dict:
        """euclidean_autoencoder.py:137-150 / spherical_vae.py:143-156: ReduceLROnPlateau with patience 2."""
        cfg = super().configure_optimizers()
        cfg["lr_scheduler"]["patience"] = 2
        return cfg


class LitAutoEncoder(_AutogradLit):
    """models/euclidean_autoencoder.py: STSAE with loss lambda_ * MSE(x_rec, x) + MSE(z, c) + alpha * reg (:106-118),
    static centre from the initial latents (:76-100), window score = reconstruction error (eval_utils.py:77-105 with its
    default loss_type 'rec').  The reference unpacks the model's outputs in the order of its missing old module
    (SURVEY 8a row a9); the intent -- first the reconstruction, then the latent -- is what is implemented."""

    from .models.sts.ae import STSAE as model_cls

    def __init__(self, args: Namespace) -> None:
        self._build(args)
        self.lambda_ = float(getattr(args, "lambda_", 0.01))

    def forward(self, x):
        z, x_rec = self.model(x[0])
        return x_rec, z, x[0], x[1], x[2], x[3]

    def setup(self, stage: str = None, train_loader=None, resume: bool = False) -> None:
        if stage != "fit":
            return
        dev = self.model.c.device
        acc = torch.zeros(ops.head_slots(self.model.latent_dim), device=dev)
        self.model.eval()
        with torch.no_grad():
            for batch in (train_loader() if not resume else ()):        # (resume: the centre comes from the checkpoint)
                z, _ = self.model(batch[0].to(dev))
                ops.mse_head(z.contiguous(), self.model.c, need_grad=False, acc=acc)
        if not resume:
            parallel.allreduce_sum_(acc)
            self.model.c.copy_(ops.center_finalize(acc, self.eps, self.model.latent_dim))
        self.model.train()
        self._make_optimiser('ae', lambda_=self.lambda_)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        x = batch[0].to(self.model.c.device, non_blocking=True)
        if self._flat is not None:
            out = self._flat.step(x)
            if batch_idx % 20 == 0 or self._reg_last is None:   # (the regulariser: evaluated when logged, reused in between)
                self._reg_last = self._flat.reg_loss().reshape(())
            loss = (self.lambda_ * out['rec'] + out['head']).reshape(()) + float(getattr(self.args, "alpha", 0.0)) * self._reg_last
            if batch_idx % 20 == 0:
                self.log("loss", loss)
                self.log("reconstruction_loss", out['rec']); self.log("hypersphere_loss", out['head'])
                self.log("regularization", self._reg_last)
            self._log_grad_norm(self._flat, batch_idx)
            return loss
        z, x_rec = self.model(x)
        loss_reco = F.mse_loss(x_rec, x)
        loss_h = F.mse_loss(z, self.model.c.expand_as(z))
        loss_reg = self._reg_loss()
        loss = self.lambda_ * loss_reco + loss_h + float(getattr(self.args, "alpha", 0.0)) * loss_reg
        self._optimise(loss)
        if batch_idx % 20 == 0:
            self.log("loss", loss.detach()); self.log("reconstruction_loss", loss_reco.detach())
            self.log("hypersphere_loss", loss_h.detach()); self.log("regularization", loss_reg.detach())
        self._log_grad_norm(self, batch_idx)
        return loss.detach()

    # score type: the wrapper's own validation calls windows_based_loss_rec_and_hy with its default 'rec'
    # (euclidean_autoencoder.py:197); eval_COSKAD.py derives 'hyp' from its rec_loss_weight = 0 (:58-66) and sets it here
    score_type = 'rec'
    rec_loss_weight = 0.2

    def window_scores_from_batch(self, x: torch.Tensor) -> torch.Tensor:
        if self.score_type == 'hyp':           # the latent alone: no decoder
            z, rec = self.model.encode(x), None
        else:                                   # the last decoder layer and the error in one launch where the kernel is built
            z, rec = self.model.reconstruction_scores(x)
        return eval_utils.rec_and_hy_from_rec(rec, z, self.model.c, self.rec_loss_weight, self.score_type)

    def _error_map_refusal(self) -> Optional[str]:
        if self.score_type == 'hyp':
            return ("score type 'hyp' has no reconstruction term (the score is the latent's distance to the centre): "
                    "`window_latent_attribution` is its map")
        return super()._error_map_refusal()

    def window_latent_attribution(self, x: torch.Tensor):
        """-> (hyp [B], grad [B, C, T, V], attr [B, T, V]) of a batch of windows, eval mode: the score's latent term hyp = mean_j (z - c)^2
        (the whole score under 'hyp', the second term under 'rec+hyp'), its gradient with respect to the input skeleton and gradient x
        input summed over the coordinates -- LitEncoder.window_attribution's adjoint chain on this model's encoder, bottleneck and
        Euclidean head (coskad_amd/attribution.py).  ValueError naming the reason outside that chain's set."""
        from . import attribution
        return attribution.window_latent_attribution(self, x)


class LitVAE(_AutogradLit):
    """models/spherical_vae.py: STSVAE with loss phi * MSE(x_rec, x) + alpha * reg + beta * KL(q || p) + gamma * mean(1/kappa)
    (:81-107), `mean_vector` = mean of the epoch's sampled latents (:110-116), window score = 1 - cos(z, mean_vector)
    of the SAMPLED latent (:76-78, 200) -- stochastic, as in the reference."""

    from .models.sts.vae import STSVAE as model_cls

    def __init__(self, args: Namespace) -> None:
        self.distribution = str(getattr(args, "distribution", "ps")).lower()
        self._build(args, distribution=self.distribution, projector=getattr(args, "projector", "linear"))
        self.phi, self.beta, self.gamma = float(args.phi), float(args.beta), float(args.gamma)
        self.warmup_counter = int(getattr(args, "warmup_epochs", 0))
        if not hasattr(self.model, "mean_vector"):
            self.model.register_buffer("mean_vector", torch.zeros(1, args.latent_dim))
        self._zsum, self._zn = None, 0

    def forward(self, x):
        z, x_rec, _ = self.model(x[0])
        return z, x_rec, x[1], x[2], x[3]

    def setup(self, stage: str = None, train_loader=None, resume: bool = False) -> None:
        if stage == "fit":
            self.model.train()
            self._make_optimiser('vae', phi=self.phi, beta=self.beta, gamma=self.gamma)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        from .models.sts.vae import kl_ps_uniform
        x = batch[0].to(self.model.c.device, non_blocking=True)
        if self._flat is not None:
            out = self._flat.step(x)
            s = out['z'].sum(0, keepdim=True)
            self._zsum = s if self._zsum is None else self._zsum + s
            self._zn += out['z'].shape[0]
            if batch_idx % 20 == 0 or self._reg_last is None:   # (the regulariser: evaluated when logged, reused in between)
                self._reg_last = self._flat.reg_loss().reshape(())
            loss = ((self.phi * out['rec'] + self.beta * out['head'] + self.gamma * out['exp']).reshape(())
                    + float(getattr(self.args, "alpha", 0.0)) * self._reg_last)
            if batch_idx % 20 == 0:
                self.log("loss", loss)
                self.log("reconstruction_loss", out['rec']); self.log("kl_loss", out['head'])
                self.log("exp_dist_loss", out['exp']); self.log("regularization", self._reg_last)
            self._log_grad_norm(self._flat, batch_idx)
            return loss
        z, x_rec, (q, p, kappa) = self.model(x)
        with torch.no_grad():
            s = z.sum(0, keepdim=True)
            self._zsum = s if self._zsum is None else self._zsum + s
            self._zn += z.shape[0]
        if self.distribution == 'normal':
            loss_kl = torch.distributions.kl.kl_divergence(q, p).sum(-1).mean()
        else:
            loss_kl = kl_ps_uniform(q, p).mean()
        loss_rec = F.mse_loss(x_rec, x)
        loss_reg = self._reg_loss()
        loss_exp = (1 / kappa).mean()
        loss = self.phi * loss_rec + float(getattr(self.args, "alpha", 0.0)) * loss_reg + self.beta * loss_kl + self.gamma * loss_exp
        self._optimise(loss)
        if batch_idx % 20 == 0:
            self.log("loss", loss.detach()); self.log("reconstruction_loss", loss_rec.detach())
            self.log("kl_loss", loss_kl.detach()); self.log("exp_dist_loss", loss_exp.detach())
            self.log("regularization", loss_reg.detach())
        self._log_grad_norm(self, batch_idx)
        return loss.detach()

    def on_train_epoch_end(self) -> None:                    # update_state (:110-116)
        if self._zn:
            zs = torch.cat([self._zsum.reshape(-1), self._zsum.new_tensor([float(self._zn)])])
            parallel.allreduce_sum_(zs)
            self.model.mean_vector.copy_((zs[:-1] / zs[-1]).reshape(1, -1))
        if self.warmup_counter > 0:
            self.warmup_counter -= 1
        self._zsum, self._zn = None, 0

    training_epoch_end = on_train_epoch_end

    def window_scores_from_batch(self, x: torch.Tensor) -> torch.Tensor:
        scores = self.model.cosine_scores(x, self.model.mean_vector)     # the Gaussian head's scoring form (one launch), or None
        if scores is not None:
            return scores
        z = self.model.sample(x)[0]            # forward's latent (its draws, in its order) without the decoder behind it
        return 1 - F.cosine_similarity(self.model.mean_vector.expand_as(z), z)


class Trainer:
    """The few pytorch_lightning.Trainer behaviours the reference relies on (train_COSKAD.py:70-85,
    eval_COSKAD.py:110-116): fit with per-epoch validation, top-k checkpoints on the monitored value,
    ReduceLROnPlateau, predict from a checkpoint.  Loaders are zero-argument callables returning an iterable of
    [x, trans, meta, frames] batches (each rank builds its own shard)."""

    def __init__(self, max_epochs: int = 1, ckpt_dir: Optional[str] = None, save_top_k: int = 2,
                 monitor: str = "validation_auc") -> None:
        self.max_epochs, self.ckpt_dir, self.save_top_k, self.monitor = max_epochs, ckpt_dir, save_top_k, monitor
        self.history: List[Dict[str, float]] = []
        self._best: List[Tuple[float, str]] = []
        # the epoch a train_loader() call is for, set before every such call (a loader that reshuffles per epoch keys on it and can
        # then be resumed); `stage`: 'setup' while the model's setup() runs (its centre pass reads the loader too), then 'fit'
        self.current_epoch, self.stage = 0, 'setup'
        self.global_step = 0               # optimiser updates so far
        self._sched = {"best": -float("inf"), "num_bad_epochs": 0, "lr": None}     # the plateau rule's state

    def fit(self, model: LitEncoder, train_loader, val_loader=None, ckpt_path: Optional[str] = None) -> None:
        """ckpt_path (or the yaml key `resume_from_checkpoint`, Lightning 1.6's name): continue the run that wrote that checkpoint,
        at the epoch after it -- model, optimiser, plateau rule, top-k list, wrapper state and torch's RNG states restored"""
        ckpt_path = ckpt_path or getattr(getattr(model, "args", None), "resume_from_checkpoint", None)
        ck = torch.load(ckpt_path, map_location="cpu", weights_only=False) if ckpt_path else None
        if ck is not None and "optimizer_states" not in ck:
            raise ValueError(f"{ckpt_path}: no `optimizer_states` (a checkpoint written before training could be resumed holds the "
                             "model only): it loads through load_checkpoint / Trainer.predict, but a run cannot continue from it")
        # DDP wrap semantics (train_COSKAD.py:75-78): every rank starts from rank 0's parameters and buffers
        parallel.broadcast_module_(model.model)
        start = 0 if ck is None else int(ck["epoch"]) + 1
        self.current_epoch, self.stage = start, 'setup'
        if ck is None:
            self._sched = {"best": -float("inf"), "num_bad_epochs": 0, "lr": None}
            model.setup("fit", train_loader)
        else:
            # Lightning restores the module after setup(): the checkpoint's buffers win, so setup skips its centre pass; the
            # state goes in place into whatever the step re-homed the parameters in
            model.setup("fit", train_loader, resume=True)
            self._restore(model, ck)
        self.stage = 'fit'
        sched = model.configure_optimizers()["lr_scheduler"]
        st = self._sched
        if st["lr"] is None:
            st["lr"] = model.learning_rate
        k = int(getattr(getattr(model, "args", None), "accumulate_grad_batches", None) or 1)
        flush = getattr(model, "flush_gradients", None)
        for epoch in range(start, self.max_epochs):
            model.model.train()
            self.current_epoch = epoch
            n = 0
            for i, batch in enumerate(train_loader()):
                model.training_step(batch, i)
                n += 1
            if flush is not None:          # a pending accumulation group: Lightning steps on the epoch's last batch
                flush()
            self.global_step += -(-n // k)
            model.on_train_epoch_end()
            rec = dict(model.logged, epoch=epoch)
            if val_loader is not None:
                auc = self.validate(model, val_loader)
                rec["validation_auc"] = auc
                if auc > st["best"]:
                    st["best"], st["num_bad_epochs"] = auc, 0
                else:
                    st["num_bad_epochs"] += 1
                    if st["num_bad_epochs"] > sched["patience"]:
                        st["lr"] = max(st["lr"] * sched["factor"], sched["min_lr"])
                        model._engine.set_lr(st["lr"])
                        st["num_bad_epochs"] = 0
                self._checkpoint(model, epoch, auc)
            elif "loss" in rec:
                # no validation: ModelCheckpoint(monitor='loss', mode='min') (train_COSKAD.py:70-73)
                self._checkpoint(model, epoch, rec["loss"], monitor="loss", mode="min")
            self.history.append(rec)

    def _restore(self, model: LitEncoder, ck: Dict) -> None:
        sd = {k[len("model."):]: v for k, v in ck["state_dict"].items() if k.startswith("model.")}
        model.model.load_state_dict(sd, strict=True)
        model.load_optimizer_state(ck["optimizer_states"][0])
        self._sched = dict(ck["lr_schedulers"][0])
        self.global_step = int(ck.get("global_step", 0))
        own = ck.get("coskad", {})
        self._best = [tuple(b) for b in own.get("best_checkpoints", [])]
        if hasattr(model, "load_resume_state"):
            model.load_resume_state(own.get("wrapper", {}))
        if own.get("rng_cpu") is not None:
            torch.set_rng_state(own["rng_cpu"])
        if own.get("rng_device") is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state(own["rng_device"])

    def validate(self, model: LitEncoder, loader) -> float:
        # Lightning's DDP wrap broadcasts rank 0's buffers (BatchNorm running statistics, the centre) before every
        # forward (broadcast_buffers=True): validation scores every shard with the model that gets checkpointed
        parallel.broadcast_buffers_(model.model)
        model.model.eval()
        outs = [model.validation_step(b, i) for i, b in enumerate(loader())]
        if parallel.world_size() > 1:
            # shards are wrap-padded to equal length (same number of collectives on every rank): gather, then drop the
            # duplicated windows -- a window is identified by (transformation, scene, clip, person, start)
            cat = [torch.cat([o[i].to(outs[0][0].device) for o in outs], 0) for i in range(4)]
            cat = [parallel.gather_rows(t) for t in cat]
            keep = parallel.dedupe_rows(torch.cat([cat[1].long().reshape(-1, 1), cat[2].long()], 1))
            outs = [tuple(t[keep] for t in cat)]
        return model.validation_epoch_end(outs)

    def predict(self, model: LitEncoder, loader, ckpt_path: Optional[str] = None):
        if ckpt_path:
            load_checkpoint(model, ckpt_path)
        model.model.eval()
        return [model.predict_step(b, i) for i, b in enumerate(loader())]

    def _checkpoint(self, model: LitEncoder, epoch: int, value: float, monitor: Optional[str] = None,
                    mode: str = "max") -> None:
        if not self.ckpt_dir or parallel.rank() != 0:
            return
        os.makedirs(self.ckpt_dir, exist_ok=True)
        path = os.path.join(self.ckpt_dir, f"epoch={epoch}-{monitor or self.monitor}={value:.4f}.ckpt")
        # the top-k list first, so that the checkpoint carries the list it belongs to (a resumed run prunes as this one would)
        self._best.append((value, path))
        self._best.sort(key=lambda t: -t[0] if mode == "max" else t[0])
        dropped, self._best = self._best[self.save_top_k:], self._best[:self.save_top_k]
        if all(p != path for _, p in dropped):
            extra = {"lr_schedulers": [dict(self._sched)], "global_step": self.global_step,
                     "coskad": {"best_checkpoints": [list(b) for b in self._best],
                                "wrapper": model.resume_state() if hasattr(model, "resume_state") else {},
                                "rng_cpu": torch.get_rng_state(),
                                "rng_device": torch.cuda.get_rng_state() if torch.cuda.is_available() else None}}
            if hasattr(model, "optimizer_state"):
                extra["optimizer_states"] = [model.optimizer_state()]
            save_checkpoint(model, path, epoch, extra)
        for _, p in dropped:
            if os.path.exists(p):
                os.remove(p)


def save_checkpoint(model: LitEncoder, path: str, epoch: int = 0, extra: Optional[Dict] = None) -> None:
    """Lightning layout: state_dict keys prefixed `model.`, hyper_parameters = the args Namespace; `extra`: what the Trainer adds
    for resuming (optimizer_states, lr_schedulers, global_step, and under `coskad` its top-k list, the wrapper's own state and
    torch's RNG states)."""
    sd = {"model." + k: v.detach().cpu().clone() for k, v in model.model.state_dict().items()}
    torch.save(dict({"state_dict": sd, "hyper_parameters": {"args": vars(model.args)}, "epoch": epoch}, **(extra or {})), path)


def load_checkpoint(model: LitEncoder, path: str) -> None:
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = {k[len("model."):]: v for k, v in ck["state_dict"].items() if k.startswith("model.")}
    model.model.load_state_dict(sd, strict=True)
