"""CPU checks of the wide-latent plumbing (16 < latent <= 512): the head slot layout, the inverse covariance from a wide
accumulator, and the C header / library exports of the new entry points."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops


def test_head_slot_layout():
    assert [ops.head_slots(L) for L in (1, 8, 16)] == [ops.HEAD_SLOTS] * 3 == [19] * 3
    assert [ops.head_slots(L) for L in (17, 32, 64, 512)] == [20, 35, 67, 515]
    assert ops.head_count_slot(16) == 17 and ops.head_count_slot(64) == 65
    with pytest.raises(ValueError):
        ops.head_slots(513)
    lib = _lib.lib()
    lib.coskad_head_slots_l.restype = ctypes.c_int
    for L in (1, 16, 17, 100, 512):
        assert lib.coskad_head_slots_l(L) == ops.head_slots(L)
    assert lib.coskad_head_slots_l(513) == 0
    lib.coskad_head_ws_floats_l.restype = ctypes.c_size_t
    lib.coskad_head_ws_floats.restype = ctypes.c_size_t
    assert lib.coskad_head_ws_floats_l(4096, 16) == lib.coskad_head_ws_floats(4096)
    assert lib.coskad_head_ws_floats_l(4096, 64) >= 67


def test_inv_cov_from_a_wide_accumulator():
    from coskad_amd.trainer import inv_cov_from_moments
    g = torch.Generator().manual_seed(0)
    L, n = 40, 300
    z = torch.randn(n, L, generator=g, dtype=torch.float64)
    acc = torch.zeros(ops.head_slots(L), dtype=torch.float32)
    acc[1:1 + L] = z.sum(0).float()
    acc[L + 1] = n
    acc[17] = -1.0        # slot 17 is a vector-sum slot at L = 40: the count must come from slot L + 1
    acc[1 + 16] = z.sum(0)[16].float()
    mu = z.mean(0).float()
    want = torch.inverse(torch.cov(z.T))
    got = inv_cov_from_moments((z.T @ z).float(), acc, mu, L)
    torch.testing.assert_close(got.double(), want, rtol=2e-3, atol=2e-3)


def test_header_declares_the_wide_entry_points():
    syms = set(_lib.header_symbols())
    for s in ("coskad_head_slots_l", "coskad_head_ws_floats_l", "coskad_btlnk_fwd_ws_bytes_l"):
        assert s in syms, s
        assert hasattr(_lib.lib(), s), s


def test_wide_shape_errors_without_a_gpu():
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    with pytest.raises(_lib.CoskadHipError, match="max 512"):
        _lib.call("coskad_mse_head_f32", p, p, null, null, p, null, ctypes.c_float(1.0), p, _lib.i32(4), _lib.i32(513), null)
    with pytest.raises(_lib.CoskadHipError, match="512"):
        _lib.call("coskad_btlnk_bwd_f32", p, p, p, null, p, p, null, null, p, ctypes.c_size_t(1 << 30), _lib.i32(0), _lib.i32(4),
                  _lib.i32(816), _lib.i32(600), null)
    lib = _lib.lib()
    lib.coskad_btlnk_fwd_ws_bytes_l.restype = ctypes.c_size_t
    lib.coskad_btlnk_fwd_ws_bytes.restype = ctypes.c_size_t
    assert lib.coskad_btlnk_fwd_ws_bytes_l(4096, 13056, 16) == lib.coskad_btlnk_fwd_ws_bytes(4096)
    assert lib.coskad_btlnk_fwd_ws_bytes_l(4096, 13056, 64) >= 4096 * 64 * 4
