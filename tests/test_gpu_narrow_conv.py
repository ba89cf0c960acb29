"""Kernel-level checks of csrc/last_layer.hip (coskad_narrow_conv_fwd_f32, coskad_narrow_conv_bwd_f32, coskad_narrow_conv_rows)
against kernel_refs.narrow_conv in double, gradients from autograd: every J in {2, 4, 6, 8}, every channel count the backward is
built for, with and without the producer's slope, at clip counts and lengths that leave partly filled waves, and one case that sends
both kernels through a second grid-stride round.  Bounds: k * U32 * M as in test_gpu_wide_kernels.py; derivations in the docstrings."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_refs import U32, U64, dd
from test_gpu_wide_kernels import _close

pytestmark = pytest.mark.gpu

A_IN = 0.2
SHAPES = [(1, 4), (3, 204), (7, 300)]          # B TV / 4 = 1, 153, 525 position quads: never a multiple of 256, two with a partly filled wave


def _rows_expected(B, TV):
    """the launcher's grid: one workgroup per 256 position quads, at most 1024"""
    return min(-(-(B * (TV // 4)) // 256), 1024)


def _inputs(B, Ci, J, TV, seed, zeros=True):
    g = torch.Generator().manual_seed(seed)
    U = torch.randn(B, Ci, 1, TV, generator=g)
    if zeros:                                      # exact +0.0 and -0.0: pins the derivative at zero to torch's (the slope's side)
        flat = U.view(-1)
        flat[0], flat[1], flat[flat.numel() // 2], flat[-1] = 0.0, -0.0, 0.0, -0.0
    W = torch.randn(J, Ci, generator=g) / Ci ** 0.5
    dOut = torch.randn(B, J, 1, TV, generator=g)
    return U, W, dOut


@pytest.mark.parametrize("Ci", [5, 16, 32, 64])
@pytest.mark.parametrize("J", [2, 4, 6, 8])
def test_narrow_conv_fwd(J, Ci):
    """out_j = sum_c w_jc PReLU(u_c) as one fma chain over the channels (Ci = 5: the remainder of the `unroll 4` loop): a term sees
    at most Ci roundings, the PReLU's a u one more -- k = Ci + 1, M = sum_c |w_jc| |x_c|."""
    from coskad_amd import _lib, ops
    for B, TV in SHAPES:
        assert _lib.lib().coskad_narrow_conv_rows(B, TV) == _rows_expected(B, TV)
        for pre in (True, False):
            U, W, _ = _inputs(B, Ci, J, TV, seed=J * 100 + Ci + B + TV)
            slope = torch.tensor([A_IN]) if pre else None
            out = ops.narrow_conv_fwd(U.cuda(), slope.cuda() if pre else None, W.cuda())
            U64_, W64 = dd(U).view(B, Ci, TV), dd(W)
            ref = R.narrow_conv(U64_, R.f32(A_IN) if pre else None, W64)
            X = R.prelu(U64_, R.f32(A_IN)) if pre else U64_
            M = torch.einsum("jc,bcp->bjp", W64.abs(), X.abs())
            _close(f"fwd J{J} Ci{Ci} B{B} TV{TV} pre{int(pre)}", out.cpu().view(B, J, TV).numpy(), ref.numpy(), ((Ci + 1) * U32 * M).numpy())


def _bwd_raw(U, slope, W, dOut):
    """ops.narrow_conv_bwd with the partial rows kept: -> (dU, rows [rows, J Ci + 1], sums [J Ci + 1])"""
    from coskad_amd import _lib, ops
    B, Ci, T, V = U.shape
    J = W.shape[0]
    rows, E = _lib.lib().coskad_narrow_conv_rows(B, T * V), J * Ci + 1
    part = torch.full((rows, E), float("nan"), device="cuda")
    dU = torch.empty_like(U)
    _lib.call("coskad_narrow_conv_bwd_f32", U, slope, W, dOut, dU, part, part.numel(), B, Ci, J, T * V, ops._stream())
    dU2, sums = ops.narrow_conv_bwd(U, slope, W, dOut)
    assert torch.equal(dU2, dU)
    return dU, part, sums, rows


def _check_bwd(tag, U, W, dOut, pre, rounds):
    """dU_c = (sum_j w_jc g_j) PReLU'(u_c): an fma chain over j and the a d product: k = J + 1, M = sum_j |w_jc g_j| (times a where
    u <= 0).
    dW_jc: x = PReLU(u) (1), the thread's four products and three adds as g.w x.w and three fma (4), wave_total's six DPP adds (6),
    `red += s` once per grid-stride round (rounds), the four-wave sum (2): k = 13 + rounds on M = sum |g_j| |x_c| for the raw rows
    summed in double by the test; coskad_gemm_sum_f32 sums in double and rounds once more: k + 1.
    Slope gradient sum (W^T g)_c u_c [u_c < 0]: d (J), d u (1), the four-term sum (3), `da +=` once per channel and round
    (Ci rounds), wave_sum (6), the four-wave sum (2): k = J + 12 + Ci rounds on M = sum (sum_j |w_jc g_j|) |u_c| [u_c < 0]."""
    B, Ci, _, TV = U.shape
    J = W.shape[0]
    slope = torch.tensor([A_IN]) if pre else None
    dU, part, sums, rows = _bwd_raw(U.cuda(), slope.cuda() if pre else None, W.cuda(), dOut.cuda())
    assert rows == _rows_expected(B, TV)
    a = torch.tensor(R.f32(A_IN), dtype=torch.float64, requires_grad=True)
    U64_ = dd(U).view(B, Ci, TV).requires_grad_(True)
    W64 = dd(W).requires_grad_(True)
    g64 = dd(dOut).view(B, J, TV)
    out = R.narrow_conv(U64_, a if pre else None, W64)
    grads = torch.autograd.grad(out, [U64_, W64] + ([a] if pre else []), g64)
    Ud, Wd = U64_.detach(), W64.detach()
    dabs = torch.einsum("jc,bjp->bcp", Wd.abs(), g64.abs())
    gate = torch.where(Ud > 0, torch.ones_like(Ud), torch.full_like(Ud, R.f32(A_IN))) if pre else torch.ones_like(Ud)
    _close(tag + " dU", dU.cpu().view(B, Ci, TV).numpy(), grads[0].numpy(), ((J + 1) * U32 * dabs * gate).numpy())
    X = R.prelu(Ud, R.f32(A_IN)) if pre else Ud
    Mw = torch.einsum("bjp,bcp->jc", g64.abs(), X.abs()).reshape(-1)
    k = 13 + rounds
    raw = part.cpu().double().sum(0)
    assert torch.isfinite(raw).all()
    _close(tag + " dW rows", raw[:-1].numpy(), grads[1].reshape(-1).numpy(), (k * U32 * Mw).numpy())
    _close(tag + " dW sums", sums.cpu()[:-1].numpy(), grads[1].reshape(-1).numpy(), ((k + 1) * U32 * Mw).numpy())
    if pre:
        Ma = float((dabs * Ud.abs())[Ud < 0].sum())
        ka = J + 12 + Ci * rounds
        _close(tag + " dslope rows", raw[-1:].numpy(), grads[2].reshape(1).numpy(), np.full(1, ka * U32 * Ma))
        _close(tag + " dslope sums", sums.cpu()[-1:].numpy(), grads[2].reshape(1).numpy(), np.full(1, (ka + 1) * U32 * Ma))
    else:
        assert float(raw[-1]) == 0.0 and float(sums[-1]) == 0.0


@pytest.mark.parametrize("Ci", [16, 32, 64])
@pytest.mark.parametrize("J", [2, 4, 6, 8])
def test_narrow_conv_bwd(J, Ci):
    """every <J, Ci> instantiation of k_narrow_bwd at the three shapes, with and without in_slope; bounds: _check_bwd"""
    for B, TV in SHAPES:
        for pre in (True, False):
            U, W, dOut = _inputs(B, Ci, J, TV, seed=J * 1000 + Ci + B + TV)
            _check_bwd(f"bwd J{J} Ci{Ci} B{B} TV{TV} pre{int(pre)}", U, W, dOut, pre, rounds=1)


def test_narrow_conv_second_grid_stride_round():
    """B = 1, Ci = 16, J = 2, TV = 4 * 262 400: 262 400 position quads against a grid of 1024 x 256 = 262 144 threads, so workgroup 0
    runs a second round on the last 256 quads and every other workgroup runs it dead (all lanes carry zeros).  About 70 MB on the
    device; forward and backward, once.  rounds = 2 in the bounds."""
    from coskad_amd import _lib, ops
    B, Ci, J, TV = 1, 16, 2, 4 * 262_400
    assert B * (TV // 4) > 1024 * 256 and _lib.lib().coskad_narrow_conv_rows(B, TV) == 1024
    U, W, dOut = _inputs(B, Ci, J, TV, seed=77)
    out = ops.narrow_conv_fwd(U.cuda(), torch.tensor([A_IN]).cuda(), W.cuda())
    U64_, W64 = dd(U).view(B, Ci, TV), dd(W)
    X = R.prelu(U64_, R.f32(A_IN))
    _close("big fwd", out.cpu().view(B, J, TV).numpy(), R.narrow_conv(U64_, R.f32(A_IN), W64).numpy(),
           ((Ci + 1) * U32 * torch.einsum("jc,bcp->bjp", W64.abs(), X.abs())).numpy())
    del out, X
    _check_bwd("big bwd", U, W, dOut, True, rounds=2)


def test_narrow_conv_rows_and_partial_table_check():
    """coskad_narrow_conv_rows is the grid the backward launches: a table of exactly that many rows is taken (every test above), one
    row fewer is refused before anything is launched; shapes the kernels do not take give 0 rows"""
    from coskad_amd import _lib, ops
    lib = _lib.lib()
    for B, TV in SHAPES + [(1, 4 * 262_400), (64, 204), (1024, 1024)]:
        assert lib.coskad_narrow_conv_rows(B, TV) == _rows_expected(B, TV), (B, TV)
    for B, TV in [(0, 204), (3, 0), (3, 51), (-1, 4)]:
        assert lib.coskad_narrow_conv_rows(B, TV) == 0
    B, Ci, J, TV = 7, 16, 4, 300
    U, W, dOut = (t.cuda() for t in _inputs(B, Ci, J, TV, seed=3))
    rows, E = lib.coskad_narrow_conv_rows(B, TV), J * Ci + 1
    assert rows == 3
    part = torch.zeros(rows, E, device="cuda")
    dU = torch.empty_like(U)
    with pytest.raises(_lib.CoskadHipError, match="partial table too small"):
        _lib.call("coskad_narrow_conv_bwd_f32", U, None, W, dOut, dU, part, (rows - 1) * E, B, Ci, J, TV, ops._stream())
