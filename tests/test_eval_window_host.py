"""CPU checks of the folded one-clip layer kernel at the window lengths 8 / 16 / 24 (csrc/eval_layer_clip.hip): the set the
library's predicate states, how plan_stack routes a stack of layers, and what the C ABI says before it touches a
device.  No kernel runs."""
import ctypes

import pytest
import torch
import torch.nn as nn

from coskad_amd import _lib, engine, ops
from coskad_amd.models.graph_layers.stsgcn import plan_stack
from coskad_amd.models.sts.ae import STSE

# every combination is built and none is switched off
SUPPORTED = {(T, V, Ci, Co) for T in (8, 16, 24) for V in (17, 25) for Ci in (16, 32) for Co in (16, 32, 64)}


def test_predicate_is_the_stated_set():
    fn = _lib.lib().coskad_layer_apply_window_ok
    seen = set()
    for T in (4, 8, 10, 12, 16, 20, 24, 32):
        for V in (14, 17, 18, 25, 26):
            for Ci in (2, 8, 16, 32, 64):
                for Co in (2, 8, 16, 32, 64, 128):
                    got = fn(T, V, Ci, Co)
                    assert got in (0, 1)
                    assert bool(got) == ((T, V, Ci, Co) in SUPPORTED), (T, V, Ci, Co)
                    assert ops.layer_apply_window_ok(T, V, Ci, Co) == bool(got)
                    seen.add((T, V, Ci, Co)) if got else None
    assert seen == SUPPORTED and len(SUPPORTED) == 36
    for V in (17, 25):
        for Ci, Co in ((16, 16), (32, 64)):
            assert fn(12, V, Ci, Co) == 0                 # T = 12 is not a "window" geometry
        for T in (10, 32):
            assert fn(T, V, 32, 32) == 0
    for T in (8, 16, 24):
        for V in (14, 18):
            assert fn(T, V, 32, 32) == 0
        for Ci in (2, 8, 64):
            assert fn(T, 17, Ci, 32) == 0
        for Co in (2, 8, 128):
            assert fn(T, 17, 32, Co) == 0


def test_first_pair_predicate():
    fn = _lib.lib().coskad_layer_first_pair_ok
    for V in (17, 25):
        for Co in (16, 32, 64):
            assert fn(12, V, 2, 32, Co) == 1              # T = 12: as before
            assert fn(12, V, 2, 16, Co) == 0
            for T in (8, 16, 24):
                assert fn(T, V, 2, 32, Co) == 1
                assert fn(T, V, 2, 16, Co) == 0 and fn(T, V, 3, 32, Co) == 0
    for T, V in ((12, 14), (12, 18), (8, 14), (16, 18), (10, 17), (32, 25)):
        assert fn(T, V, 2, 32, 32) == 0
    assert fn(8, 17, 2, 32, 8) == 0 and fn(8, 17, 2, 32, 128) == 0


def _encoder_layers(T, V=17, channels=(32, 16, 32), hid=64, latent=16):
    torch.manual_seed(0)
    m = STSE(2, list(channels), hid, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    return m, list(m.encoder.model)


def test_plan_default_encoder():
    m, layers = _encoder_layers(8)
    m.eval()
    assert plan_stack(layers, False) == [("window_eval", 0, 4)]
    assert plan_stack(layers, True) == [("wide", i, i + 1) for i in range(4)]           # somebody needs a gradient
    m.train()
    assert plan_stack(layers, False) == [("wide", i, i + 1) for i in range(4)]           # batch statistics
    m.eval()
    engine.EVAL_WINDOW = False
    try:
        assert plan_stack(layers, False) == [("wide", i, i + 1) for i in range(4)]
    finally:
        engine.EVAL_WINDOW = True
    engine.EVAL_FIRST_PAIR = False
    try:
        assert plan_stack(layers, False) == [("wide", 0, 1), ("window_eval", 1, 4)]      # a lone 2 -> 32 layer stays composed
    finally:
        engine.EVAL_FIRST_PAIR = True
    assert plan_stack(layers, False) == [("window_eval", 0, 4)]
    for T, V in ((16, 25), (24, 17), (24, 25)):
        m, layers = _encoder_layers(T, V)
        m.eval()
        assert plan_stack(layers, False) == [("window_eval", 0, 4)], (T, V)


def test_plan_narrow_encoder():
    m, layers = _encoder_layers(8, channels=(16, 8, 16), hid=16, latent=8)
    m.eval()
    assert [(l.in_channels, l.out_channels) for l in layers] == [(2, 16), (16, 8), (8, 16), (16, 16)]
    assert plan_stack(layers, False) == [("wide", 0, 1), ("wide", 1, 2), ("wide", 2, 3), ("window_eval", 3, 4)]


def test_plan_other_joint_layouts_stay_composed():
    m, layers = _encoder_layers(16, V=18)
    m.eval()
    assert plan_stack(layers, False) == [("wide", i, i + 1) for i in range(4)]


def test_plan_batchnorm_without_running_statistics():
    m, layers = _encoder_layers(8)
    layers[2].tcn[1] = nn.BatchNorm2d(32, track_running_stats=False)
    layers[2].residual[1] = nn.BatchNorm2d(32, track_running_stats=False)
    m.eval()
    assert plan_stack(layers, False) == [("window_eval", 0, 2), ("wide", 2, 3), ("window_eval", 3, 4)]
    layers[1].tcn[1] = nn.BatchNorm2d(16, track_running_stats=False)
    layers[1].residual[1] = nn.BatchNorm2d(16, track_running_stats=False)
    m.eval()
    # (the 2 -> 32 head has lost its partner)
    assert plan_stack(layers, False) == [("wide", 0, 1), ("wide", 1, 2), ("wide", 2, 3), ("window_eval", 3, 4)]


def test_plan_at_12_frames_is_a_chain():
    m, layers = _encoder_layers(12)
    m.eval()
    assert plan_stack(layers, False) == [("chain", 0, 4)]
    assert plan_stack(layers, True) == [("chain", 0, 4)]
    m.train()
    assert plan_stack(layers, True) == [("chain", 0, 4)]


def _aligned(n_floats):
    """a host buffer and a 16-byte aligned address inside it"""
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_argument_checks_come_before_the_device():
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    odd = ctypes.c_void_p(a + 4)

    def apply(inp, out, B=1, T=8, V=17, Ci=32, Co=32, A=p):
        _lib.call("coskad_layer_apply_f32", inp, out, A, p, p, p, null, null, B, Ci, Co, T, V, null)

    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        apply(null, p)
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        apply(p, p, A=null)
    for B in (0, -3):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*B=" + str(B)):
            apply(p, p, B=B)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`in`.*16-byte aligned"):
        apply(odd, p)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`out`.*16-byte aligned"):
        apply(p, odd)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\).*unsupported"):
        apply(p, p, Ci=8)                                  # 8 channels at 8 frames: no one-launch layer, no tile kernel
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\).*unsupported"):
        apply(p, p, V=14)

    def pair(x, out, B=1, T=8, V=17, Cm=32, Co=32):
        _lib.call("coskad_layer_first_pair_apply_f32", x, out, p, p, p, p, p, p, p, p, p, null, B, Cm, Co, T, V, null)

    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        pair(null, p)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`x`.*16-byte aligned"):
        pair(odd, p)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`out`.*16-byte aligned"):
        pair(p, odd, T=24, V=25, Co=64)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\).*built for"):
        pair(p, p, B=0)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\).*built for"):
        pair(p, p, Cm=16)
