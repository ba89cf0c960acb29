"""Host-side checks of the decoder models at latents beyond 16 (autoencoder and spherical VAE on the flat step): which models
`STSAETrainStep.supports` admits, the argument refusals of the widened entry points (nothing is launched here), and the Python
predicates against the library's."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops, trainer
from coskad_amd.models.sts.ae import STSAE
from coskad_amd.models.sts.vae import STSVAE


def _ae(latent, projector='linear'):
    return STSAE(2, [32, 16, 32], 64, latent, 12, 17, 'sts_gcn', projector, 'euclidean', 0.0)


def _vae(latent, projector='linear', distribution='ps'):
    return STSVAE(2, [32, 16, 32], 64, latent, 12, 17, 'sts_gcn', projector, 'euclidean', 0.0, distribution=distribution)


def test_supports_admits_latents_up_to_512():
    sup = trainer.STSAETrainStep.supports
    for L in (17, 32, 512):
        assert sup(_ae(L)), L
    assert not sup(_ae(513))
    for L in (32, 511):
        assert sup(_vae(L)), L
    assert not sup(_vae(512))                    # 512 mean rows + the concentration row
    assert sup(_vae(64, projector='mlp')) and _vae(64, projector='mlp').btlnk.hidden_layers == [64]
    assert not sup(_vae(65, projector='mlp'))    # hidden width 65: beyond csrc/mlp_head.hip
    # the Gaussian head stacks 2 L rows; it stays a matter of the latent stage (_AutogradLatent)
    assert sup(_vae(32, distribution='normal')) and sup(_vae(256, distribution='normal'))
    assert not sup(_vae(257, distribution='normal'))
    assert not sup(_ae(32, projector='mlp'))     # the autoencoder's flat step takes the `linear` projector only


def test_supports_at_narrow_latents_is_unchanged():
    sup = trainer.STSAETrainStep.supports
    for L in (2, 8, 12, 16):
        assert sup(_ae(L)) and not sup(_ae(L, projector='mlp'))
    for L in (2, 8, 15):
        assert sup(_vae(L))
    for L in (4, 8, 16):
        assert sup(_vae(L, projector='mlp'))
    assert not sup(_vae(16))                     # 17 stacked rows: beyond the narrow bottleneck kernel, as before
    assert sup(_vae(8, distribution='normal')) and not sup(_vae(9, distribution='normal'))
    assert sup(_vae(8, 'mlp', 'normal'))


def test_a_measured_off_latent_leaves_supports(monkeypatch):
    monkeypatch.setattr(ops, "AE_WIDE_OFF", frozenset({32}))
    assert not trainer.STSAETrainStep.supports(_ae(32)) and trainer.STSAETrainStep.supports(_ae(64))
    assert not trainer.STSAETrainStep.supports(_vae(32))


def test_make_decoder_step_takes_wide_latents_when_asked():
    """the wrappers ask (`flat_wide_latent`, default on); without the flag a latent beyond 16 stays on the autograd route"""
    torch.manual_seed(0)
    assert trainer.make_decoder_step(_ae(32).train(), 'ae', lr=0.0) is None
    eng = trainer.make_decoder_step(_ae(32).train(), 'ae', wide_latent=True, lr=0.0)
    assert type(eng) is trainer.STSAETrainStep and type(eng.entry) is trainer._PlainEntry and eng.lowrank is None
    assert eng.center_acc.shape == (ops.head_slots(32),)
    eng = trainer.make_decoder_step(_vae(24).train(), 'vae', wide_latent=True, lr=0.0)
    assert type(eng.projector) is trainer._StackedHeads and type(eng.latent) is trainer._PowerSphericalLatent
    assert type(trainer.make_decoder_step(_vae(24, distribution='normal').train(), 'vae', wide_latent=True, lr=0.0).latent) \
        is trainer._AutogradLatent
    assert type(trainer.make_decoder_step(_ae(8).train(), 'ae', lr=0.0)) is trainer.STSAETrainStep
    with pytest.raises(TypeError, match="head rows <= 512"):
        trainer.STSAETrainStep(_ae(513).train(), mode='ae')


def _p():
    buf = (ctypes.c_float * 16)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_ps_head_argument_errors_are_reported_without_a_gpu():
    keep, p = _p()
    null = ctypes.c_void_p(0)
    E = _lib.CoskadHipError
    for L in (1, 513):
        with pytest.raises(E, match="ps_head_prep: B=4 latent=%d" % L):
            _lib.call("coskad_ps_head_prep_f32", p, 600, p, 600, p, p, p, p, 4, L, None)
        with pytest.raises(E, match="ps_head_sample: B=4 latent=%d" % L):
            _lib.call("coskad_ps_head_sample_f32", p, p, p, p, p, p, p, 4, L, None)
        with pytest.raises(E, match="ps_head_bwd: B=4 latent=%d" % L):
            _lib.call("coskad_ps_head_bwd_f32", p, p, p, p, p, p, p, 600, p, 600, 0.1, 0.1, p, 600, p, 600, 4, L, None)
    for L in (8, 64):                                      # a row stride below the latent is a shape error at either width
        with pytest.raises(E, match="ps_head_prep"):
            _lib.call("coskad_ps_head_prep_f32", p, L - 1, p, 1, p, p, p, p, 4, L, None)
        with pytest.raises(E, match="null pointer"):
            _lib.call("coskad_ps_head_prep_f32", null, L, p, 1, p, p, p, p, 4, L, None)
        with pytest.raises(E, match="null pointer"):
            _lib.call("coskad_ps_head_sample_f32", p, p, p, p, null, p, p, 4, L, None)
        with pytest.raises(E, match="null pointer"):
            _lib.call("coskad_ps_head_bwd_f32", p, p, p, p, p, p, p, L, p, 1, 0.1, 0.1, p, L, null, 1, 4, L, None)
    del keep


def test_ps_head_error_codes():
    """COSKAD_ERR_SHAPE (-2) for the latent, COSKAD_ERR_ARG (-1) for a null pointer: straight from the library"""
    keep, p = _p()
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    for L in (1, 513):
        assert lib.coskad_ps_head_prep_f32(p, 600, p, 600, p, p, p, p, 4, L, None) == -2
        assert lib.coskad_ps_head_sample_f32(p, p, p, p, p, p, p, 4, L, None) == -2
        assert lib.coskad_ps_head_bwd_f32(p, p, p, p, p, p, p, 600, p, 600, 0.1, 0.1, p, 600, p, 600, 4, L, None) == -2
    assert lib.coskad_ps_head_prep_f32(null, 600, p, 600, p, p, p, p, 4, 64, None) == -1
    assert lib.coskad_ps_head_sample_f32(p, p, p, p, p, null, p, 4, 64, None) == -1
    assert lib.coskad_ps_head_bwd_f32(p, p, p, p, p, p, p, 600, p, 600, 0.1, 0.1, null, 600, p, 600, 4, 64, None) == -1
    del keep


def test_rev_btlnk_argument_errors_are_reported_without_a_gpu():
    keep, p = _p()
    E = _lib.CoskadHipError
    for N, L in ((816, 513), (816, 12), (818, 64), (818, 16)):
        with pytest.raises(E, match=f"rev_btlnk_fwd: B=4 N={N} L={L}"):
            _lib.call("coskad_rev_btlnk_fwd_f32", p, p, p, p, 4, N, L, None)
        with pytest.raises(E, match=f"rev_btlnk_bwd: B=4 N={N} L={L}"):
            _lib.call("coskad_rev_btlnk_bwd_f32", p, p, p, p, 0, p, p, 0, p, 4, N, L, None)
        assert _lib.lib().coskad_rev_btlnk_fwd_f32(p, p, p, p, 4, N, L, None) == -2
    with pytest.raises(E, match="null pointer"):
        _lib.call("coskad_rev_btlnk_fwd_f32", None, p, p, p, 4, 816, 64, None)
    del keep


def test_rev_btlnk_predicates():
    lib = _lib.lib()
    for L in (8, 12, 16, 17, 64, 512, 513):
        for N in (816, 818):
            assert ops.rev_btlnk_wide_ok(N, L) == bool(lib.coskad_rev_btlnk_wide_ok(N, L)) == (16 < L <= 512 and N == 816), (N, L)
            assert ops.rev_btlnk_ok(N, L) == (L in (8, 16) and N == 816), (N, L)          # as before
            assert not (ops.rev_btlnk_ok(N, L) and ops.rev_btlnk_wide_ok(N, L))
    # the workspace of the wide backward: the larger of the dz partials (slices of N x [B, L]) and the dW / db partials
    assert lib.coskad_rev_btlnk_ws_floats(4096, 13056, 512) >= 13056 * 513
    assert lib.coskad_rev_btlnk_ws_floats(37, 13056, 16) == 13056 * 17 * 2                 # narrow latents: as before (2 slices)
    assert ops.PS_HEAD_LMAX == 512
