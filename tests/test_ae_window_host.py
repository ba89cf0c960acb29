"""CPU checks of the decoder models' training route at the window lengths 8 / 16 / 24: the few-channel predicate the
library states and its Python restatement, the older predicate beside it, how STSAETrainStep cuts the two stacks with and without
`fused_window`, and what the C ABI says about a few-channel layer it does not serve before it touches a device.  No kernel runs."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops, trainer
from coskad_amd.models.sts.ae import STSAE
from coskad_amd.models.sts.vae import STSVAE

NARROW = {(T, V, 4, 2) for T in (8, 16, 24) for V in (17, 25)}


def test_narrow_predicate_is_the_stated_set():
    fn = _lib.lib().coskad_layer_train_window_narrow_ok
    seen = set()
    for T in (8, 12, 16, 24):
        for V in (14, 17, 18, 25):
            for Ci in (2, 4, 6, 8, 16):
                for Co in (1, 2, 3, 4, 16):
                    got = fn(T, V, Ci, Co)
                    assert got in (0, 1)
                    assert bool(got) == ((T, V, Ci, Co) in NARROW), (T, V, Ci, Co)
                    assert ops.layer_train_window_narrow_ok(T, V, Ci, Co) == bool(got), (T, V, Ci, Co)
                    if got:
                        seen.add((T, V, Ci, Co))
    assert seen == NARROW and len(seen) == 6
    for T in (10, 11, 32):
        assert fn(T, 17, 4, 2) == 0 and not ops.layer_train_window_narrow_ok(T, 17, 4, 2)
    assert "coskad_layer_train_window_narrow_ok" in _lib.header_symbols()
    assert not ops.TRAIN_WINDOW_NARROW_OFF and not ops.TRAIN_WINDOW_OFF     # nothing switched off in Python


def test_wide_predicate_keeps_its_set():
    fn = _lib.lib().coskad_layer_train_window_ok
    ones = 0
    for T in (8, 12, 16, 24):
        for V in (14, 17, 18, 25):
            for Ci in (2, 4, 8, 16, 32, 64):
                for Co in (2, 4, 8, 16, 32, 64):
                    got = fn(T, V, Ci, Co)
                    assert ops.layer_train_window_ok(T, V, Ci, Co) == bool(got)
                    if Co <= 4 or Ci == 4:
                        assert got == 0, (T, V, Ci, Co)
                    ones += got
    assert ones == 54


def _ae(T, V=17, channels=(32, 16, 32), hid=64, latent=16):
    torch.manual_seed(0)
    return STSAE(c_in=2, h_dim=hid, latent_dim=latent, n_frames=T, n_joints=V, dropout=0.0, channels=list(channels)).train()


def _kinds(stack):
    return [s.kind for s in stack.segs]


@pytest.mark.parametrize("T,V", [(8, 17), (16, 25), (24, 17)])
def test_default_widths_cut_into_window_runs_and_a_narrow_layer(T, V):
    eng = trainer.STSAETrainStep(_ae(T, V), fused_window=True)
    assert _kinds(eng.enc) == ['window'] and len(eng.enc.segs[0].layers) == 4
    assert eng.lowrank is not None
    assert _kinds(eng.dec) == ['window', 'narrow'] and len(eng.dec.segs[0].layers) == 2
    assert isinstance(eng.dec.segs[1], trainer._NarrowLayer)
    assert (eng.dec.segs[1].virt.Ci, eng.dec.segs[1].virt.Co) == (4, 2)
    assert eng.enc.top([None]) == (None, None)
    # who writes which PReLU gradient: the window run writes the folded layer's, the narrow layer the window run's, the head the last
    gv = eng.fp.gviews
    assert eng.dec.segs[0].out_slope_grad is gv["decoder.model.2.prelu.weight"]
    assert eng.dec.last_slope_grad is gv["decoder.model.3.prelu.weight"]
    assert eng.enc.last_slope_grad is gv["encoder.model.3.prelu.weight"]
    assert trainer.STSAETrainStep.segment_kinds(_ae(T, V), fused_window=True) == (['window'] * 4, ['window', 'window', 'narrow'])
    # off unless asked for: both stacks composed, ending in activated outputs -- a cut the step refuses before it touches the model
    for kw in ({}, dict(fused_window=False)):
        assert trainer.STSAETrainStep.segment_kinds(_ae(T, V), **kw) == (['wide'] * 4, ['wide'] * 3)
        with pytest.raises(NotImplementedError, match="STSAETrainStep: an encoder ending in a wide layer"):
            trainer.STSAETrainStep(_ae(T, V), **kw)


def test_vae_cuts_the_same_way():
    torch.manual_seed(0)
    m = STSVAE(c_in=2, h_dim=64, latent_dim=8, n_frames=8, n_joints=17, dropout=0.0, channels=[32, 16, 32], distribution='ps',
               projector='linear').train()
    eng = trainer.STSAETrainStep(m, mode='vae', fused_window=True)
    assert _kinds(eng.enc) == ['window'] and _kinds(eng.dec) == ['window', 'narrow'] and eng.lowrank is not None


def test_twelve_frames_unchanged_by_the_flag():
    for V in (17, 25):
        a, b = trainer.STSAETrainStep(_ae(12, V)), trainer.STSAETrainStep(_ae(12, V), fused_window=True)
        assert _kinds(a.enc) == _kinds(b.enc) and _kinds(a.dec) == _kinds(b.dec)
        assert 'window' not in _kinds(b.enc) + _kinds(b.dec) and _kinds(b.dec)[-1] == 'narrow'
        assert type(b.dec.segs[-1]) is type(a.dec.segs[-1])


def test_mixed_stacks_keep_wide_segments():
    # 8-channel layers have no window kernels; a joint layout without them keeps every layer composed
    eng = trainer.STSAETrainStep(_ae(8, 17, channels=(16, 8, 16), hid=16), fused_window=True)
    assert 'wide' in _kinds(eng.enc) and 'wide' in _kinds(eng.dec)
    enc_k, dec_k = trainer.STSAETrainStep.segment_kinds(_ae(8, 17, channels=(16, 8, 16), hid=16), fused_window=True)
    assert enc_k == ['window', 'wide', 'wide', 'window'] == _kinds(eng.enc) and 'wide' in dec_k       # (per layer)
    enc_k, dec_k = trainer.STSAETrainStep.segment_kinds(_ae(16, 18), fused_window=True)
    assert set(enc_k + dec_k) == {'wide'}
    with pytest.raises(NotImplementedError, match="STSAETrainStep: an encoder ending in a wide layer"):
        trainer.STSAETrainStep(_ae(16, 18), fused_window=True)
    # a last layer with dropout stays composed: a decoder ending in an activated output, which the step refuses
    m = _ae(8, 17)
    m.decoder.model[-1].dropout = 0.1
    assert trainer.STSAETrainStep.segment_kinds(m, fused_window=True)[1] == ['window', 'window', 'wide']
    with pytest.raises(NotImplementedError, match="STSAETrainStep: a decoder ending in a wide layer"):
        trainer.STSAETrainStep(m, fused_window=True)


def _aligned(n_floats):
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_unserved_few_channel_shapes_are_refused_before_the_device():
    """(4 -> 2) at 11 frames and (6 -> 3) at 8 frames: COSKAD_ERR_SHAPE (-2) from every entry point of the layer, nothing launched; the
    alignment of the activations is still judged first at a window geometry"""
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p, odd = ctypes.c_void_p(a), ctypes.c_void_p(a + 4)
    big = 1 << 40
    err = _lib.CoskadHipError

    def stats_z(inp, Z, T, V, Ci, Co):
        _lib.call("coskad_layer_train_stats_z_f32", inp, p, p, null, p, p, p, p, p, p, p, p, p, p, p, p, p, p,
                  0.1, p, p, p, p, big, 1, Ci, Co, T, V, null, Z)

    def apply_z(Z, inp, out, T, V, Ci, Co):
        _lib.call("coskad_layer_apply_z_f32", Z, inp, out, p, p, p, p, null, null, 1, Ci, Co, T, V, null)

    def bwd_z(inp, dU, Z, T, V, Ci, Co, dIn=p):
        _lib.call("coskad_layer_bwd_z_f32", inp, dU, p, p, null, p, p, p, p, p, dIn, p, p, p, p, p, p, p, p, p, p,
                  null, p, big, 0, 1, Ci, Co, T, V, null, Z)

    for T, V, Ci, Co, text in ((11, 17, 4, 2, r"unsupported \(n_frames=11"), (8, 17, 6, 3, "unsupported")):
        with pytest.raises(err, match=r"failed \(-2\).*" + text):
            stats_z(p, p, T, V, Ci, Co)
        with pytest.raises(err, match=r"failed \(-2\).*" + text):
            bwd_z(p, p, p, T, V, Ci, Co)
    with pytest.raises(err, match=r"failed \(-2\).*unsupported \(n_frames=11"):
        apply_z(p, p, p, 11, 17, 4, 2)
    # the served shape: alignment first, by name, then the workspace -- still nothing launched
    with pytest.raises(err, match=r"failed \(-1\).*layer_train_stats: `in`.*16-byte aligned"):
        stats_z(odd, p, 8, 17, 4, 2)
    with pytest.raises(err, match=r"failed \(-1\).*layer_bwd: `dIn`.*16-byte aligned"):
        bwd_z(p, p, p, 8, 17, 4, 2, dIn=odd)
    with pytest.raises(err, match=r"failed \(-1\).*layer_bwd: `Z`.*16-byte aligned"):
        bwd_z(p, p, odd, 8, 17, 6, 3)
    L = _lib.lib()
    L.coskad_layer_bwd_ws_bytes.restype = ctypes.c_size_t
    for T, V, B in ((8, 17, 1), (24, 25, 7)):
        need = L.coskad_layer_bwd_ws_bytes(B, 4, 2, T, V)
        assert need > 2 * B * 4 * T * V * 4                                   # dZ and dX_res live there
        with pytest.raises(err, match=r"failed \(-4\).*workspace"):
            _lib.call("coskad_layer_bwd_z_f32", p, p, p, p, null, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p,
                      null, p, need - 1, 0, B, 4, 2, T, V, null, p)
    del buf
