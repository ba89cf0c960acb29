"""Resuming a run from a checkpoint (Trainer.fit(ckpt_path=...)): 4 epochs straight against 2 epochs, then a fresh model and
Trainer resumed from the epoch-1 checkpoint up to 4.  The kernels are deterministic and the loader reshuffles per epoch keyed on
Trainer.current_epoch, so the two runs agree bit for bit."""
import glob
import os

import pytest
import torch

from test_gpu_end_to_end import make_args

pytestmark = pytest.mark.gpu

_data = {}


def data():
    from coskad_amd.utils.synthetic import make_dataset
    if not _data:
        _data["train"], _ = make_dataset(n_scenes=2, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=False, seed=1)
        _data["test"], _data["gts"] = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=True,
                                                   seed=2)
    return _data["train"], _data["test"], _data["gts"]


def fit(cls, args, ckpt_dir, max_epochs, ckpt_path=None):
    from coskad_amd.lit import Trainer
    from coskad_amd.utils.synthetic import batches
    train, test, gts = data()
    torch.manual_seed(0)
    lit = cls(args).cuda()
    lit.gts = gts
    tr = Trainer(max_epochs=max_epochs, ckpt_dir=str(ckpt_dir), save_top_k=8)

    def train_loader():                 # reshuffled per epoch; setup's centre pass takes permutation 0
        return batches(train, 128, shuffle=True, seed=0, epoch=0 if tr.stage == 'setup' else tr.current_epoch + 1)

    tr.fit(lit, train_loader, lambda: batches(test, 512), ckpt_path=ckpt_path)
    return lit, tr


def step_of(lit):
    return lit._flat if getattr(lit, "_flat", None) is not None else lit._engine


def straight_and_resumed(cls, args, tmp_path):
    a, ta = fit(cls, args, tmp_path / "a", 4)
    _, tb = fit(cls, args, tmp_path / "b", 2)
    (path,) = glob.glob(os.path.join(str(tmp_path / "b"), "epoch=1-*.ckpt"))
    c, tc = fit(cls, args, tmp_path / "c", 4, ckpt_path=path)
    return (a, ta), (c, tc), path


def assert_same_run(straight, resumed):
    (a, ta), (c, tc) = straight, resumed
    assert [h["epoch"] for h in tc.history] == [2, 3]
    assert tc.history == ta.history[2:], (ta.history[2:], tc.history)
    sa, sc = a.model.state_dict(), c.model.state_dict()
    assert all(torch.equal(sa[k], sc[k]) for k in sa), [k for k in sa if not torch.equal(sa[k], sc[k])]
    ea, ec = step_of(a), step_of(c)
    assert torch.equal(ea.m, ec.m) and torch.equal(ea.v, ec.v) and ea.updates == ec.updates > 0
    assert ea._bpow == ec._bpow and tc.global_step == ta.global_step and tc._sched == ta._sched


@pytest.mark.parametrize("mode", ["euclid_dynamic", "hyperbolic"])
def test_encoder_resume_is_bit_identical(mode, tmp_path):
    from coskad_amd.lit import LitEncoder
    from coskad_amd.trainer import STSETrainStep
    # (hyperbolic: clipped and accumulated, so `grad_norm` is logged before the epoch's first update and has to cross the resume)
    clip = dict(gradient_clip_val=1.0, accumulate_grad_batches=2) if mode == "hyperbolic" else {}
    args = make_args(hyperbolic=mode == "hyperbolic", **clip)
    straight, resumed, _ = straight_and_resumed(LitEncoder, args, tmp_path)
    assert type(resumed[0]._engine) is STSETrainStep
    assert_same_run(straight, resumed)
    if mode == "hyperbolic":
        assert "grad_norm" in resumed[1].history[-1]


def test_autoencoder_resume_is_bit_identical(tmp_path):
    from coskad_amd.lit import LitAutoEncoder
    args = make_args(latent_dim=8, lambda_=0.01, decoder_channels=[8, 8], use_decoder=True, accumulate_grad_batches=2)
    straight, resumed, _ = straight_and_resumed(LitAutoEncoder, args, tmp_path)
    assert resumed[0]._flat is not None
    assert_same_run(straight, resumed)


def test_vae_resume_restores_optimiser_and_generators(tmp_path):
    """the sampler draws from torch's device generator only, whose state the checkpoint carries: the resumed run is the straight one"""
    from coskad_amd.lit import LitVAE
    args = make_args(latent_dim=8, phi=1.0, beta=1e-3, gamma=1e-2, distribution="ps", warmup_epochs=1, decoder_channels=[8, 8],
                     use_vae=True)
    straight, resumed, path = straight_and_resumed(LitVAE, args, tmp_path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["coskad"]["rng_device"] is not None and ck["coskad"]["wrapper"]["warmup_counter"] == 0
    assert resumed[0]._flat is not None
    assert resumed[1].history[0]["loss"] == straight[1].history[2]["loss"]
    assert_same_run(straight, resumed)


def test_checkpoint_without_optimizer_states(tmp_path):
    from coskad_amd.lit import LitEncoder, Trainer, load_checkpoint, save_checkpoint
    from coskad_amd.utils.synthetic import batches
    train, _, _ = data()
    lit = LitEncoder(make_args(validation=False)).cuda()
    path = str(tmp_path / "model_only.ckpt")
    save_checkpoint(lit, path, 0)
    with pytest.raises(ValueError, match="optimizer_states"):
        Trainer(max_epochs=2).fit(LitEncoder(make_args(validation=False)).cuda(), lambda: batches(train, 128), ckpt_path=path)
    fresh = LitEncoder(make_args(validation=False)).cuda()
    load_checkpoint(fresh, path)
    assert all(torch.equal(v, fresh.model.state_dict()[k]) for k, v in lit.model.state_dict().items())
