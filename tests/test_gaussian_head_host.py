"""Host-side checks of the Gaussian VAE head (`distribution: 'normal'`, csrc/vae_head_normal.hip): the header's three entry points and
their binding, the latent predicate against the library's, the argument refusals (nothing is launched here), which latent stage the
decoder step picks with and without `gaussian_head`, and the yaml."""
import argparse
import ctypes
import os

import pytest
import torch
import yaml

from coskad_amd import _lib, ops, trainer
from coskad_amd.models.sts.vae import STSVAE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"coskad_normal_head_ok": 1, "coskad_normal_head_fwd_f32": 14, "coskad_normal_head_bwd_f32": 16}


def _vae(latent, projector='linear', distribution='normal'):
    torch.manual_seed(0)
    return STSVAE(2, [32, 16, 32], 64, latent, 12, 17, 'sts_gcn', projector, 'euclidean', 0.0, distribution=distribution).train()


def test_header_declares_and_library_exports_the_three_entry_points():
    protos = _lib.prototypes()
    lib = _lib.lib()
    for name, n in NARGS.items():
        assert name in protos, name
        restype, argtypes = protos[name]
        assert restype is ctypes.c_int and len(argtypes) == n, (name, len(argtypes))
        assert hasattr(lib, name) and _lib._nargs[name] == n
    with pytest.raises(TypeError, match="takes 14 arguments"):
        _lib.call("coskad_normal_head_fwd_f32", None)


def test_normal_head_ok_agrees_with_the_library():
    lib = _lib.lib()
    for L in (0, 1, 16, 17, 512, 513):
        assert ops.normal_head_ok(L) == bool(lib.coskad_normal_head_ok(L)) == (1 <= L <= 512), L
    assert ops.NORMAL_HEAD_LMAX == 512 and ops.NORMAL_HEAD_OFF == frozenset()


def _p():
    buf = (ctypes.c_float * 16)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_normal_head_refusals_come_before_any_launch():
    """COSKAD_ERR_SHAPE (-2) for the latent (and B = 0, as the ps_head entries), COSKAD_ERR_ARG (-1) naming the argument otherwise"""
    keep, p = _p()
    lib, null, E = _lib.lib(), ctypes.c_void_p(0), _lib.CoskadHipError
    fwd = lambda *a: lib.coskad_normal_head_fwd_f32(*a, None)
    bwd = lambda *a: lib.coskad_normal_head_bwd_f32(*a, None)
    for L in (0, 513):
        assert fwd(p, 600, p, 600, p, p, p, p, p, null, null, 4, L) == -2
        assert bwd(p, p, p, p, 600, p, 600, 0.1, 0.1, p, 600, p, 600, 4, L) == -2
        with pytest.raises(E, match=f"normal_head_fwd: latent={L}"):
            _lib.call("coskad_normal_head_fwd_f32", p, 600, p, 600, p, p, p, p, p, None, None, 4, L, None)
        with pytest.raises(E, match=f"normal_head_bwd: latent={L}"):
            _lib.call("coskad_normal_head_bwd_f32", p, p, p, p, 600, p, 600, 0.1, 0.1, p, 600, p, 600, 4, L, None)
    assert fwd(p, 8, p, 8, p, p, p, p, p, null, null, 0, 8) == -2 and bwd(p, p, p, p, 8, p, 8, 0.1, 0.1, p, 8, p, 8, 0, 8) == -2
    assert fwd(p, 8, p, 8, p, p, p, p, p, null, null, -1, 8) == -1 and bwd(p, p, p, p, 8, p, 8, 0.1, 0.1, p, 8, p, 8, -1, 8) == -1
    cases = [("ld_mean=7", (p, 7, p, 8, p, p, p, p, p, None, None, 4, 8)),
             ("ld_var=7", (p, 8, p, 7, p, p, p, p, p, None, None, 4, 8)),
             ("score without ref", (p, 8, p, 8, p, p, p, p, p, None, p, 4, 8)),
             ("neither z nor score", (p, 8, p, 8, p, None, p, p, p, p, None, 4, 8)),
             ("null pointer", (None, 8, p, 8, p, p, p, p, p, None, None, 4, 8)),
             ("null pointer", (p, 8, p, 8, None, p, p, p, p, None, None, 4, 8))]
    for what, args in cases:
        with pytest.raises(E, match=r"normal_head_fwd_f32 failed \(-1\): normal_head_fwd: " + what):
            _lib.call("coskad_normal_head_fwd_f32", *args, None)
    cases = [("ld_mean=7", (p, p, p, p, 7, p, 8, 0.1, 0.1, p, 8, p, 8, 4, 8)),
             ("ld_var=7", (p, p, p, p, 8, p, 7, 0.1, 0.1, p, 8, p, 8, 4, 8)),
             ("ld_dmean=7", (p, p, p, p, 8, p, 8, 0.1, 0.1, p, 7, p, 8, 4, 8)),
             ("ld_dvar=7", (p, p, p, p, 8, p, 8, 0.1, 0.1, p, 8, p, 7, 4, 8)),
             ("null pointer", (p, p, None, p, 8, p, 8, 0.1, 0.1, p, 8, p, 8, 4, 8)),
             ("null pointer", (p, p, p, p, 8, p, 8, 0.1, 0.1, p, 8, None, 8, 4, 8))]
    for what, args in cases:
        with pytest.raises(E, match=r"normal_head_bwd_f32 failed \(-1\): normal_head_bwd: " + what):
            _lib.call("coskad_normal_head_bwd_f32", *args, None)
    del keep


STEPS = [   # latent, projector, wide_latent, projector form, the latent head applies the two small heads (tests/test_flat_stack_host.py)
    (8, 'linear', False, "_StackedHeads", False),
    (24, 'linear', True, "_StackedHeads", False),
    (8, 'mlp', False, "_MLPProjector", True),
]


@pytest.mark.parametrize("latent,projector,wide,form,heads", STEPS, ids=[f"{r[1]}-{r[0]}" for r in STEPS])
def test_decoder_step_takes_the_gaussian_latent_when_asked(latent, projector, wide, form, heads):
    step = trainer.make_decoder_step(_vae(latent, projector), 'vae', gaussian_head=True, wide_latent=wide, lr=0.0)
    assert type(step) is trainer.STSAETrainStep and type(step.projector) is getattr(trainer, form)
    assert type(step.latent) is trainer._GaussianLatent and step.latent.heads is heads
    names = ("fc_mean.weight", "fc_mean.bias", "fc_var.weight", "fc_var.bias") if heads else ()
    assert len(step.latent.head_params) == len(step.latent.head_grads) == 4 * heads
    for n, p, g in zip(names, step.latent.head_params, step.latent.head_grads):
        assert p is step.model.get_parameter(n) and g is step.fp.gviews[n]
        off = step.fp.offsets[n]                     # views of the two flat buffers
        assert p.data_ptr() == step.fp.flat[off:].data_ptr() and g.data_ptr() == step.fp.grad[off:].data_ptr()
    # the keyword passed to the constructor directly decides the same way
    assert type(trainer.STSAETrainStep(_vae(latent, projector), mode='vae', lr=0.0, gaussian_head=True).latent) is trainer._GaussianLatent


@pytest.mark.parametrize("latent,projector,wide,form,heads", STEPS, ids=[f"{r[1]}-{r[0]}" for r in STEPS])
def test_without_the_keyword_the_head_stays_on_autograd(latent, projector, wide, form, heads):
    step = trainer.make_decoder_step(_vae(latent, projector), 'vae', wide_latent=wide, lr=0.0)
    assert type(step.latent) is trainer._AutogradLatent and step.latent.heads is heads
    assert type(trainer.STSAETrainStep(_vae(latent, projector), mode='vae', lr=0.0).latent) is trainer._AutogradLatent


def test_the_keyword_leaves_the_other_models_alone(monkeypatch):
    step = trainer.make_decoder_step(_vae(8, distribution='ps'), 'vae', gaussian_head=True, lr=0.0)
    assert type(step.latent) is trainer._PowerSphericalLatent
    from coskad_amd.models.sts.ae import STSAE
    ae = STSAE(2, [32, 16, 32], 64, 8, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0).train()
    assert type(trainer.make_decoder_step(ae, 'ae', gaussian_head=True, lr=0.0).latent) is trainer._CentreLatent
    # a (projector, latent range) a measurement switched off keeps the autograd head
    monkeypatch.setattr(ops, "NORMAL_HEAD_OFF", frozenset({('linear', 1, 8)}))
    assert type(trainer.make_decoder_step(_vae(8), 'vae', gaussian_head=True, lr=0.0).latent) is trainer._AutogradLatent
    assert type(trainer.make_decoder_step(_vae(8, 'mlp'), 'vae', gaussian_head=True, lr=0.0).latent) is trainer._GaussianLatent


def test_gaussian_yaml_loads_through_the_argparser():
    from coskad_amd import lit
    from coskad_amd.utils.argparser import init_sub_args
    raw = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "gaussian_vae.yaml")), Loader=yaml.FullLoader)
    ps = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "spherical_vae.yaml")), Loader=yaml.FullLoader)
    assert {k for k in raw if raw[k] != ps.get(k)} == {"distribution", "dir_name"} and set(raw) == set(ps)
    args = argparse.Namespace(**raw)
    args.exp_dir = "/tmp/coskad_contract"           # nothing is written: the wrapper only reads it
    args, *_ = init_sub_args(args)
    assert args.use_vae and str(args.distribution).lower() == 'normal'
    m = lit.LitVAE(args)
    assert m.model.distribution == 'normal' and m.distribution == 'normal'
    assert m.model.fc_var.out_features == m.model.latent_dim == raw["latent_dim"]
    assert tuple(m.model.mean_vector.shape) == (1, raw["latent_dim"])
