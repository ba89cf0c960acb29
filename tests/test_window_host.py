"""CPU checks of the window lengths beside 12 (dataset_seg_len 8 / 16 / 24): the host predicate of the library and its Python
restatement, how a layer and a model of such a window length are routed (composed path only), and what the C ABI says before it
touches a device.  No kernel runs."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops, trainer
from coskad_amd.models.graph_layers.stsgcn import ST_GCNN_layer
from coskad_amd.models.sts.ae import STSE

WINDOWS = {(T, V) for T in (8, 16, 24) for V in (14, 17, 18, 25)}


def test_window_ok_is_the_stated_set():
    fn = _lib.lib().coskad_window_ok
    fn.restype = ctypes.c_int
    for T in range(4, 33):
        for V in (14, 17, 18, 25, 26):
            want = (T, V) in WINDOWS
            assert bool(fn(_lib.i32(T), _lib.i32(V))) == want, (T, V)
            assert ops.window_ok(T, V) == want, (T, V)
    assert not ops.window_ok(12, 17)          # the tile kernels' own geometry is not a "window" geometry


def test_workspace_query():
    fn = _lib.lib().coskad_gcn_bwd_params_ws_bytes
    fn.restype = ctypes.c_size_t
    for V in (14, 17, 18, 25):
        assert fn(_lib.i32(12), _lib.i32(V)) == 1024 * (12 * V * V + V * 144) * 4      # T = 12: as it was
    for T, V in sorted(WINDOWS):
        E = T * V * V + V * T * T
        rows, rem = divmod(fn(_lib.i32(T), _lib.i32(V)), 4 * E)
        assert rem == 0 and rows in (256, 512), (T, V, rows)       # one partial row per workgroup of the persistent grid
    assert fn(_lib.i32(24), _lib.i32(25)) == 256 * 29400 * 4


def _layer(T, V=17, ci=32, co=16, dropout=0.0):
    return ST_GCNN_layer(ci, co, (1, 1), 1, T, V, dropout)


def test_layer_routing():
    assert _layer(8).is_wide is True
    assert _layer(16, 25).is_wide is True and _layer(24, 14, 2, 32).is_wide is True
    # at 12 frames: what it was (tile kernels up to 64 channels while a clip fits the LDS, no dropout)
    assert _layer(12).is_wide is False
    assert _layer(12, 25, 64, 32).is_wide is True
    assert _layer(12, 17, 32, 128).is_wide is True
    assert _layer(12, dropout=0.1).is_wide is True


@pytest.mark.parametrize("T,V", [(10, 17), (12, 26), (8, 26), (32, 17)])
def test_unsupported_geometry_raises_at_construction(T, V):
    with pytest.raises(ValueError, match=r"unsupported.*\[8, 12, 16, 24\].*\[14, 17, 18, 25\]"):
        _layer(T, V)
    with pytest.raises(ValueError, match="unsupported"):
        STSE(2, [32, 16, 32], 64, 16, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)


def test_flat_stack_of_an_8_frame_encoder_is_wide_only():
    torch.manual_seed(0)
    m = STSE(2, [32, 16, 32], 64, 8, 8, 17, 'sts_gcn', 'linear', 'euclidean', 0.0).train()
    eng = trainer.make_train_step(m, lr=0.0, use_graph=True, side_stream=True)      # (both dropped, as for the wide stack)
    assert type(eng) is trainer.STSETrainStep and eng.use_graph is False and eng.side is None
    assert [s.kind for s in eng.stack.segs] == ['wide'] * 4
    assert eng.stack.last_slope_grad is None and eng.layers == []
    with pytest.raises(ValueError, match="wide layers runs on the main stream"):
        trainer.STSETrainStep(m, lr=0.0, use_graph=True)


def test_argument_checks_come_before_the_geometry():
    null = ctypes.c_void_p(0)
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        _lib.call("coskad_gcn_f32", null, null, null, null, _lib.i32(4), _lib.i32(8), _lib.i32(17), _lib.i32(0), null)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for T, V in ((11, 17), (8, 26), (20, 25)):
        with pytest.raises(_lib.CoskadHipError, match=r"unsupported.*\{8,12,16,24\}"):
            _lib.call("coskad_gcn_f32", p, p, p, p, _lib.i32(4), _lib.i32(T), _lib.i32(V), _lib.i32(0), null)
    with pytest.raises(_lib.CoskadHipError, match="workspace too small"):
        _lib.call("coskad_gcn_bwd_params_dx_f32", p, p, p, p, p, p, p, null, p, ctypes.c_size_t(64), _lib.i32(0), _lib.i32(4),
                  _lib.i32(8), _lib.i32(17), null)
