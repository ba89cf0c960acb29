"""CPU checks of the training contract around the step (coskad_amd.lit.Trainer, the wrappers' yaml keys): a pure-Python stub model
drives Trainer.fit -- no native library, no kernel."""
import shutil
from argparse import Namespace

import pytest
import torch

from coskad_amd import lit
from coskad_amd.lit import Trainer, load_checkpoint


class Stub:
    """what Trainer.fit asks of a wrapper, recording the order of the calls"""
    learning_rate = 1e-2

    def __init__(self, aucs, patience=0, **args):
        self.args = Namespace(**args)
        self.model = torch.nn.Linear(2, 1)
        torch.nn.init.zeros_(self.model.weight); torch.nn.init.zeros_(self.model.bias)
        self.logged, self.calls, self.aucs, self.patience = {}, [], list(aucs), patience
        self.lr, self.opt_step, self._epoch = self.learning_rate, 0, 0
        self._engine = self

    def setup(self, stage, train_loader, resume=False):
        self.calls.append(("setup", resume))
        if not resume:
            list(train_loader())               # the centre pass

    def set_lr(self, lr):
        self.lr = lr

    def training_step(self, batch, i):
        self.calls.append(("step", i))
        self.logged["loss"] = 1.0
        with torch.no_grad():
            self.model.weight.add_(1.0)

    def flush_gradients(self):
        self.calls.append(("flush",))
        self.opt_step += 1

    def on_train_epoch_end(self):
        self.calls.append(("epoch_end",))
        self._epoch += 1

    def configure_optimizers(self):
        return {"lr_scheduler": {"patience": self.patience, "factor": 0.5, "min_lr": 1e-6}}

    def validation_step(self, b, i):
        return b

    def validation_epoch_end(self, outs):
        return self.aucs[self._epoch - 1]

    def optimizer_state(self):
        return {"state": {}, "param_groups": [{"lr": self.lr}], "coskad": {"opt_step": self.opt_step}}

    def load_optimizer_state(self, sd):
        self.lr, self.opt_step = sd["param_groups"][0]["lr"], sd["coskad"]["opt_step"]

    def resume_state(self):
        return {"_epoch": self._epoch}

    def load_resume_state(self, st):
        self._epoch = st["_epoch"]


def loaders(tr, seen):
    def train():
        seen.append((tr.stage, tr.current_epoch))
        return [[torch.zeros(1)]] * 3
    return train, lambda: [[torch.zeros(1)]]


AUCS = [0.5, 0.7, 0.6, 0.55, 0.65]


def test_flush_once_per_epoch_and_current_epoch_before_every_loader_call(tmp_path):
    m = Stub(AUCS, accumulate_grad_batches=2)
    tr = Trainer(max_epochs=2, ckpt_dir=str(tmp_path))
    seen = []
    tr.fit(m, *loaders(tr, seen))
    assert seen == [("setup", 0), ("fit", 0), ("fit", 1)]
    epoch = [("step", 0), ("step", 1), ("step", 2), ("flush",), ("epoch_end",)]
    assert m.calls == [("setup", False)] + epoch + epoch
    assert tr.global_step == 4                        # ceil(3 / 2) updates per epoch


def test_checkpoint_keys(tmp_path):
    m = Stub(AUCS)
    tr = Trainer(max_epochs=2, ckpt_dir=str(tmp_path))
    tr.fit(m, *loaders(tr, []))
    path = dict((p.split("epoch=")[1][0], p) for _, p in tr._best)["1"]
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert {"state_dict", "hyper_parameters", "epoch", "optimizer_states", "lr_schedulers", "global_step", "coskad"} <= set(ck)
    assert all(k.startswith("model.") for k in ck["state_dict"]) and ck["epoch"] == 1 and ck["global_step"] == 6
    assert isinstance(ck["optimizer_states"], list) and len(ck["optimizer_states"]) == 1
    assert set(ck["lr_schedulers"][0]) == {"best", "num_bad_epochs", "lr"}
    assert {"best_checkpoints", "wrapper", "rng_cpu", "rng_device"} <= set(ck["coskad"])
    assert ck["coskad"]["wrapper"] == {"_epoch": 2} and len(ck["coskad"]["best_checkpoints"]) == 2
    fresh = Stub(AUCS)
    load_checkpoint(fresh, path)                      # signature and behaviour as before
    assert torch.equal(fresh.model.weight, m.model.weight)


def test_resume_restores_trainer_state_and_continues(tmp_path):
    straight = Stub(AUCS)
    ts = Trainer(max_epochs=5, ckpt_dir=str(tmp_path / "a"), save_top_k=2)
    ts.fit(straight, *loaders(ts, []))
    first = Stub(AUCS)
    t1 = Trainer(max_epochs=3, ckpt_dir=str(tmp_path / "b"), save_top_k=2)
    t1.fit(first, *loaders(t1, []))
    # epoch 2 (auc 0.6) fell out of the top 2 ({0.7, 0.5} -> {0.7, 0.6}: it is in): resume from it
    path = [p for _, p in t1._best if "epoch=2" in p][0]
    path = shutil.copy(path, str(tmp_path / "resume.ckpt"))      # (the continued run prunes its top-k list, this file included)
    m = Stub(AUCS)
    tr = Trainer(max_epochs=5, ckpt_dir=str(tmp_path / "b"), save_top_k=2)
    seen = []
    tr.fit(m, *loaders(tr, seen), ckpt_path=path)
    assert m.calls[0] == ("setup", True) and seen == [("fit", 3), ("fit", 4)]        # no centre pass; continues at epoch 3
    assert [r["epoch"] for r in tr.history] == [3, 4]
    assert tr.history == ts.history[3:]
    assert tr._sched == ts._sched and tr.global_step == ts.global_step == 15
    assert m.lr == straight.lr and m.lr < Stub.learning_rate                         # the plateau reductions carried over
    assert m.opt_step == straight.opt_step and torch.equal(m.model.weight, straight.model.weight)
    assert [(v, p.split("/")[-1]) for v, p in tr._best] == [(v, p.split("/")[-1]) for v, p in ts._best]
    # yaml key of Lightning 1.6
    m2 = Stub(AUCS, resume_from_checkpoint=path)
    t2 = Trainer(max_epochs=4, ckpt_dir=str(tmp_path / "c"))
    t2.fit(m2, *loaders(t2, []))
    assert [r["epoch"] for r in t2.history] == [3]


def test_checkpoint_without_optimizer_state_does_not_resume(tmp_path):
    m = Stub(AUCS)
    path = str(tmp_path / "old.ckpt")
    lit.save_checkpoint(m, path, 1)                   # what a checkpoint held before: state_dict, hyper_parameters, epoch
    assert set(torch.load(path, weights_only=False)) == {"state_dict", "hyper_parameters", "epoch"}
    tr = Trainer(max_epochs=3)
    with pytest.raises(ValueError, match="optimizer_states"):
        tr.fit(Stub(AUCS), *loaders(tr, []), ckpt_path=path)
    load_checkpoint(Stub(AUCS), path)


def make_args(**kw):
    """the small model of the end-to-end tests"""
    a = dict(num_coords=2, h_dim=16, latent_dim=8, dataset_seg_len=12, dropout=0, channels=[16, 8, 16], projector="linear",
             encoder_type="STS_GCN", hyperbolic=False, static_center=False, center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6,
             dataset_batch_size=256, dataset_num_transform=2, dataset_headless=False, dataset_kp18_format=False, smoothing=50,
             dataset_choice="UBnormal", validation=True)
    a.update(kw)
    return Namespace(**a)


def test_yaml_keys_reach_the_step_constructor(monkeypatch):
    args = Namespace(gradient_clip_val=1.0, gradient_clip_algorithm="value", accumulate_grad_batches=2)
    assert lit.step_knobs(args) == {"grad_clip_val": 1.0, "grad_clip_algorithm": "value", "accumulate": 2}
    assert lit.step_knobs(Namespace()) == {"grad_clip_val": 0.0, "grad_clip_algorithm": "norm", "accumulate": 1}
    assert lit.step_knobs(Namespace(gradient_clip_val=None, gradient_clip_algorithm=None, accumulate_grad_batches=None)) \
        == lit.step_knobs(Namespace())
    got = {}
    monkeypatch.setattr(lit, "make_train_step", lambda model, **kw: got.update(kw) or "step")
    enc = lit.LitEncoder(make_args(hyperbolic=True, gradient_clip_val=1.0, accumulate_grad_batches=2))
    enc.setup("fit", None, resume=True)               # builds the step only
    assert enc._engine == "step"
    assert (got["grad_clip_val"], got["grad_clip_algorithm"], got["accumulate"], got["head"]) == (1.0, "norm", 2, "poincare")
    # the decoder wrappers hand the same keywords to make_decoder_step (the flat step, asked for when the model is on the device) ...
    from coskad_amd import trainer
    seen = {}
    monkeypatch.setattr(trainer, "make_decoder_step", lambda model, mode, **kw: seen.update(kw))
    ae = lit.LitAutoEncoder(make_args(gradient_clip_val=0.5, gradient_clip_algorithm="value", accumulate_grad_batches=3))
    monkeypatch.setattr(ae, "_on_device", lambda: True)
    ae._make_optimiser('ae', lambda_=0.1)
    assert (seen["grad_clip_val"], seen["grad_clip_algorithm"], seen["accumulate"]) == (0.5, "value", 3)
    # ... and keep them for the autograd route, which a model on the host takes
    host = lit.LitAutoEncoder(make_args(gradient_clip_val=0.5, gradient_clip_algorithm="value", accumulate_grad_batches=3))
    host._make_optimiser('ae', lambda_=0.1)
    assert host._flat is None and host._opt is not None
    assert host.clip_val == 0.5 and host.clip_mode == "value" and host._knobs["accumulate"] == 3
    with pytest.raises(ValueError):
        lit.LitAutoEncoder(make_args(accumulate_grad_batches=0.5))._make_optimiser('ae')
