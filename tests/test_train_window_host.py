"""CPU checks of the stored-Z training route at the window lengths 8 / 16 / 24 (csrc/train_window_moments.hip,
csrc/train_window_flat.hip): the set the library's predicate states and its Python restatement, how the flat stack cuts
an encoder into segments with and without `fused_window`, and what the C ABI says before it touches a device.  No kernel runs."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops, trainer
from coskad_amd.models.sts.ae import STSE

SUPPORTED = {(T, V, Ci, Co) for T in (8, 16, 24) for V in (17, 25) for Ci in (2, 16, 32) for Co in (16, 32, 64)}
# the (T, V, C_in -> C_out) shapes of the default stack 2-32-16-32-64 at 17 joints
DEFAULT_STACK = [(T, 17, Ci, Co) for T in (8, 16, 24) for Ci, Co in ((2, 32), (32, 16), (16, 32), (32, 64))]


def test_predicate_is_the_stated_set():
    fn = _lib.lib().coskad_layer_train_window_ok
    seen = set()
    for T in (8, 12, 16, 24):
        for V in (14, 17, 18, 25):
            for Ci in (2, 8, 16, 32, 64):
                for Co in (2, 8, 16, 32, 64):
                    got = fn(T, V, Ci, Co)
                    assert got in (0, 1)
                    if T == 12 or V in (14, 18) or 8 in (Ci, Co) or Ci == 64 or Co <= 4:
                        assert got == 0, (T, V, Ci, Co)
                    assert bool(got) == ((T, V, Ci, Co) in SUPPORTED), (T, V, Ci, Co)
                    assert ops.layer_train_window_ok(T, V, Ci, Co) == bool(got), (T, V, Ci, Co)
                    seen.add((T, V, Ci, Co)) if got else None
    assert seen == SUPPORTED and len(SUPPORTED) == 54
    assert len(DEFAULT_STACK) == 12 and all(fn(*s) == 1 for s in DEFAULT_STACK)
    for T in (10, 11, 32):
        assert fn(T, 17, 32, 32) == 0 and not ops.layer_train_window_ok(T, 17, 32, 32)
    assert not ops.TRAIN_WINDOW_OFF                     # nothing switched off in Python: the agreement above is the whole set


def _stse(T, V=17, channels=(32, 16, 32), hid=64, latent=16):
    torch.manual_seed(0)
    return STSE(2, list(channels), hid, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0).train()


def _kinds(eng):
    return [s.kind for s in eng.stack.segs]


def test_default_stack_is_one_window_run_when_asked():
    m = _stse(8)
    eng = trainer.make_train_step(m, fused_window=True, lr=1e-3, alpha=1e-6, head='euclidean', use_graph=True, side_stream=True)
    assert type(eng) is trainer.STSETrainStep and _kinds(eng) == ['window']
    assert not eng.use_graph and eng.side is None and eng.sync_group is None     # eager, main stream: dropped as for wide stacks
    seg = eng.stack.segs[0]
    assert isinstance(seg, trainer._WindowRun) and isinstance(seg, trainer._TileRun) and len(seg.layers) == 4
    assert seg.side is None and seg.sync is None
    assert eng.stack.last_slope_grad is eng.fp.gviews["encoder.model.3.prelu.weight"]
    assert eng.stack.top([None]) == (None, None)
    for kw in (dict(use_graph=True), dict(side_stream=True)):
        with pytest.raises(ValueError, match="main stream"):
            trainer.STSETrainStep(_stse(8), fused_window=True, **kw)
    # off unless asked for
    for kw in ({}, dict(fused_window=False)):
        eng = trainer.make_train_step(_stse(8), lr=1e-3, **kw)
        assert _kinds(eng) == ['wide'] * 4 and eng.stack.last_slope_grad is None
    for T, V in ((16, 17), (24, 17), (8, 25), (24, 25)):
        assert _kinds(trainer.make_train_step(_stse(T, V), fused_window=True, lr=1e-3)) == ['window'], (T, V)
    assert _kinds(trainer.make_train_step(_stse(16, 18), fused_window=True, lr=1e-3)) == ['wide'] * 4


def test_narrow_stack_mixes_window_and_wide():
    m = _stse(8, channels=(16, 8, 16), hid=16, latent=8)
    assert [(l.in_channels, l.out_channels) for l in m.encoder.model] == [(2, 16), (16, 8), (8, 16), (16, 16)]
    eng = trainer.make_train_step(m, fused_window=True, lr=1e-3)
    assert _kinds(eng) == ['window', 'wide', 'wide', 'window']
    assert [len(s.layers) for s in eng.stack.segs if s.kind == 'window'] == [1, 1]
    assert eng.stack.last_slope_grad is eng.fp.gviews["encoder.model.3.prelu.weight"]
    assert eng.stack.segs[0].out_slope_grad is eng.fp.gviews["encoder.model.0.prelu.weight"]


def test_dropout_and_mismatched_batchnorms_stay_composed():
    torch.manual_seed(0)
    m = STSE(2, [32, 16, 32], 64, 16, 8, 17, 'sts_gcn', 'linear', 'euclidean', 0.1).train()
    assert _kinds(trainer.make_train_step(m, fused_window=True, lr=1e-3)) == ['wide'] * 4
    m = _stse(8)
    m.encoder.model[1].residual[1].momentum = 0.3        # the two BatchNorms of a layer share one statistics kernel
    assert _kinds(trainer.make_train_step(m, fused_window=True, lr=1e-3)) == ['window', 'wide', 'window']


def test_twelve_frames_unchanged_by_the_flag():
    a = trainer.make_train_step(_stse(12), lr=1e-3)
    b = trainer.make_train_step(_stse(12), fused_window=True, lr=1e-3)
    assert _kinds(a) == _kinds(b) == ['tile']
    assert type(b.stack.segs[0]) is trainer._TileRun and len(b.layers) == 4


def test_fusion_probes_are_zero_beside_twelve_frames():
    for T in (8, 16, 24):
        for V in (17, 25):
            for Ci, Co in ((2, 32), (32, 16), (16, 32), (32, 64), (16, 16), (32, 32)):
                assert not ops.layer_apply_next_ok(Ci, Co, T, V)
                assert not ops.layer_apply_next_flat_ok(Ci, Co, T, V)
                for below in (2, 16, 32):
                    assert ops.layer_bwd_below_rows(4, Ci, Co, below, T, V) == 0


def _aligned(n_floats):
    """a host buffer and a 16-byte aligned address inside it"""
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_argument_checks_come_before_the_device():
    """null pointers and sizes, then the alignment of the activations (by name), then the shape -- all before anything is launched"""
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    odd = ctypes.c_void_p(a + 4)
    L = _lib.lib()
    L.coskad_layer_bwd_ws_bytes.restype = ctypes.c_size_t
    L.coskad_train_stats_ws_bytes.restype = ctypes.c_size_t
    big = 1 << 40

    def stats_z(inp, Z, B=1, T=8, V=17, Ci=16, Co=None, ws_bytes=big):
        Co = Ci if Co is None else Co
        r = p if Ci != Co else null                      # a residual convolution with its BatchNorm where the widths differ
        _lib.call("coskad_layer_train_stats_z_f32", inp, p, p, null, p, p, p, p, p, p, p, r, r, r, r, r, r, r,
                  0.1, p, p, p, p, ws_bytes, B, Ci, Co, T, V, null, Z)

    def moments(inp, Z, B=1, T=8, V=17, Ci=16, sums=p):
        _lib.call("coskad_layer_train_moments_f32", inp, p, p, null, Z, sums, p, big, B, Ci, T, V, null)

    def apply_z(Z, inp, out, B=1, T=8, V=17, Ci=16, Co=16, **_):
        _lib.call("coskad_layer_apply_z_f32", Z, inp, out, p, p, p, p, null, null, B, Ci, Co, T, V, null)

    def bwd_z(inp, dU, Z, dIn=p, B=1, T=8, V=17, Ci=16, Co=None, ws_bytes=big):
        Co = Ci if Co is None else Co
        r = p if Ci != Co else null
        _lib.call("coskad_layer_bwd_z_f32", inp, dU, p, p, null, p, p, p, r, r, dIn, p, p, p, p, p, p, r, r, r, r,
                  null, p, ws_bytes, 0, B, Ci, Co, T, V, null, Z)

    def bwd_chain(inp, dU, Z, B=1, T=8, V=17, Ci=16, Co=None, below_stats=null):
        Co = Ci if Co is None else Co
        r = p if Ci != Co else null
        _lib.call("coskad_layer_bwd_chain_f32", inp, dU, p, p, null, p, p, p, r, r, p, p, p, p, p, p, p, r, r, r, r,
                  null, p, big, 0, B, Ci, Co, T, V, null, Z, null, 0, 0, p, p, null, 2, below_stats, big, 0.0)

    def bwd_stats(inp, dU, Z, B=1, T=8, V=17, Ci=16, Co=16):
        rows = ctypes.c_int(0)
        _lib.call("coskad_layer_bwd_stats_f32", inp, dU, p, p, null, 0, p, big, ctypes.byref(rows), p, big, B, Ci, Co, T, V, null, Z)

    err = _lib.CoskadHipError
    # 1. null pointers and B <= 0 come first, also beside a misaligned pointer
    with pytest.raises(err, match="null pointer"):
        stats_z(null, odd)
    with pytest.raises(err, match="null pointer"):
        moments(odd, p, sums=null)
    with pytest.raises(err, match="null pointer"):
        apply_z(null, odd, p)
    with pytest.raises(err, match="null pointer"):
        bwd_z(odd, null, p)
    with pytest.raises(err, match="null pointer"):
        bwd_chain(odd, p, null)
    with pytest.raises(err, match="null pointer"):
        bwd_stats(odd, null, p)
    for B in (0, -3):
        for call in (lambda: stats_z(odd, p, B=B), lambda: moments(odd, p, B=B), lambda: apply_z(p, odd, p, B=B),
                     lambda: bwd_z(odd, p, p, B=B), lambda: bwd_chain(p, odd, p, B=B), lambda: bwd_stats(p, p, odd, B=B)):
            with pytest.raises(err, match=r"failed \(-1\).*B=" + str(B)):
                call()
    # 2. a misaligned activation is named, at every window geometry -- also one whose shape is not served
    for kw in ({}, dict(Ci=8), dict(T=24, V=25, Ci=32), dict(V=14)):
        with pytest.raises(err, match=r"failed \(-1\).*layer_train_stats: `in`.*16-byte aligned"):
            stats_z(odd, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_train_stats: `Z`.*16-byte aligned"):
            stats_z(p, odd, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_train_moments: `in`.*16-byte aligned"):
            moments(odd, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_train_moments: `Z`.*16-byte aligned"):
            moments(p, odd, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_apply_z: `Z`.*16-byte aligned"):
            apply_z(odd, p, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_apply_z: `in`.*16-byte aligned"):
            apply_z(p, odd, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_apply_z: `out`.*16-byte aligned"):
            apply_z(p, p, odd, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_bwd: `in`.*16-byte aligned"):
            bwd_z(odd, p, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_bwd: `dU`.*16-byte aligned"):
            bwd_z(p, odd, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_bwd: `Z`.*16-byte aligned"):
            bwd_z(p, p, odd, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_bwd: `dIn`.*16-byte aligned"):
            bwd_z(p, p, p, dIn=odd, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_bwd_chain: `dU`.*16-byte aligned"):
            bwd_chain(p, odd, p, **kw)
        with pytest.raises(err, match=r"failed \(-1\).*layer_bwd_stats: `Z`.*16-byte aligned"):
            bwd_stats(p, p, odd, **kw)
    # 3. then the shape: 8 channels at 8 frames have neither these kernels nor tile kernels; 11 frames keep the old text
    for call in (stats_z, moments):
        with pytest.raises(err, match=r"failed \(-2\).*unsupported"):
            call(p, p, Ci=8)
        with pytest.raises(err, match=r"failed \(-2\).*unsupported \(n_frames=11"):
            call(odd, p, T=11)
    with pytest.raises(err, match=r"failed \(-2\).*unsupported"):
        apply_z(p, p, p, Ci=8)
    with pytest.raises(err, match=r"failed \(-2\).*unsupported \(n_frames=11"):
        apply_z(p, p, p, Ci=16, T=11)
    for call in (bwd_z, bwd_chain, bwd_stats):
        with pytest.raises(err, match=r"failed \(-2\).*unsupported"):
            call(p, p, p, Ci=8)
        with pytest.raises(err, match=r"failed \(-2\).*unsupported \(n_frames=11"):
            call(p, p, p, T=11)
    # the layer below's reductions are not formed beside 12 frames
    with pytest.raises(err, match=r"failed \(-2\).*cannot form the reductions"):
        bwd_chain(p, p, p, Ci=32, Co=16, below_stats=p)
    # 4. the workspace: the query answers for the new route, and one byte less is refused before anything is launched
    for T, V, Ci, Co, B in ((8, 17, 16, 16, 1), (24, 25, 32, 64, 7), (16, 17, 2, 32, 3)):
        need = L.coskad_layer_bwd_ws_bytes(B, Ci, Co, T, V)
        assert need > 2 * B * Ci * T * V * 4                                  # dZ and dX_res live there
        with pytest.raises(err, match=r"failed \(-4\).*workspace"):
            bwd_z(p, p, p, B=B, T=T, V=V, Ci=Ci, Co=Co, ws_bytes=need - 1)
        need = L.coskad_train_stats_ws_bytes(Ci)
        with pytest.raises(err, match=r"failed \(-4\).*workspace"):
            stats_z(p, p, B=B, T=T, V=V, Ci=Ci, Co=Co, ws_bytes=need - 1)
    del buf
