"""coskad_prelu_fwd_f32, coskad_narrow_conv_fwd_f32 and coskad_narrow_conv_bwd_f32 move 16-byte vectors through the caller's
pointers; ops._chk asks only for contiguity, which a view at a 4-byte offset satisfies.  The C ABI refuses such a pointer by name
before anything is launched (COSKAD_ERR_ARG), like coskad_layer_tail_f32 / coskad_layer_apply_f32 / coskad_layer_train_moments_f32.
Host pointers stand in for device ones: every call here is refused before a kernel could see them.  No kernel runs."""
import ctypes

import pytest

from coskad_amd import _lib

ERR = _lib.CoskadHipError


def _aligned(n_floats):
    """a host buffer and a 16-byte aligned address inside it"""
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_prelu_fwd_refuses_misaligned_pointers():
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    for off in (4, 8, 12):
        odd = ctypes.c_void_p(a + off)
        with pytest.raises(ERR, match=r"failed \(-1\).*prelu_fwd: `u`.*16-byte aligned"):
            _lib.call("coskad_prelu_fwd_f32", odd, p, p, 16, null)
        with pytest.raises(ERR, match=r"failed \(-1\).*prelu_fwd: `out`.*16-byte aligned"):
            _lib.call("coskad_prelu_fwd_f32", p, p, odd, 16, null)
    with pytest.raises(ERR, match=r"failed \(-1\).*prelu_fwd: `u`.*16-byte aligned"):
        _lib.call("coskad_prelu_fwd_f32", ctypes.c_void_p(a + 4), p, p, 3, null)       # fewer than four elements: the same contract
    with pytest.raises(ERR, match=r"failed \(-1\).*prelu_fwd: bad argument"):
        _lib.call("coskad_prelu_fwd_f32", null, p, p, 16, null)
    with pytest.raises(ERR, match=r"failed \(-1\).*prelu_fwd: bad argument"):
        _lib.call("coskad_prelu_fwd_f32", ctypes.c_void_p(a + 4), p, p, 0, null)       # the null / empty check comes first


def test_narrow_conv_refuses_misaligned_pointers():
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    odd = ctypes.c_void_p(a + 4)

    def fwd(U=p, out=p, slope=null, B=1, Ci=16, J=4, TV=4):
        _lib.call("coskad_narrow_conv_fwd_f32", U, slope, p, out, B, Ci, J, TV, null)

    def bwd(U=p, dOut=p, dU=p, slope=null, B=1, Ci=16, J=4, TV=4, floats=65):
        _lib.call("coskad_narrow_conv_bwd_f32", U, slope, p, dOut, dU, p, floats, B, Ci, J, TV, null)

    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_fwd: `U`.*16-byte aligned"):
        fwd(U=odd)
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_fwd: `out`.*16-byte aligned"):
        fwd(out=odd)
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_fwd: `U`.*16-byte aligned"):
        fwd(U=odd, J=3)                                    # the pointer is judged before the shape
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_fwd: null pointer"):
        fwd(U=null)
    with pytest.raises(ERR, match=r"failed \(-2\).*narrow_conv_fwd: B=1 Ci=16 J=3"):
        fwd(J=3)
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_bwd: `U`.*16-byte aligned"):
        bwd(U=odd)
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_bwd: `dOut`.*16-byte aligned"):
        bwd(dOut=odd)
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_bwd: `dU`.*16-byte aligned"):
        bwd(dU=odd)
    with pytest.raises(ERR, match=r"failed \(-1\).*narrow_conv_bwd: `dU`.*16-byte aligned"):
        bwd(dU=odd, floats=0)                              # ... and before the partial table
    with pytest.raises(ERR, match=r"narrow_conv_bwd: partial table too small"):
        bwd(floats=64)
    with pytest.raises(ERR, match=r"failed \(-2\).*narrow_conv_bwd: built for 16 / 32 / 64"):
        bwd(Ci=5, floats=21)
    # the slope, the weights and the partial table are read and written as scalars: no alignment asked of them
    with pytest.raises(ERR, match=r"failed \(-2\).*narrow_conv_fwd: B=1 Ci=16 J=3"):
        fwd(slope=odd, J=3)
