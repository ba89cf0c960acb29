"""ops.btlnk_fwd with the bottleneck forward's operands staged through LDS (csrc/bottleneck.hip, k_btlnk_fwd_t: whole-line buffer loads
of U and W per group of four k-steps, a wave-private LDS image, a branch-free main loop and a guarded tail): z against the float64
torch expression PReLU(U) @ W^T + b, and a repeat call byte-equal.

The tolerance is the one of the existing float64 test of this kernel, test_gpu_btlnk_kernels.test_narrow_forward_split_k:
|z - ref| <= k_fwd_split(K, KS, pre, bias) * U32 * M,  M = |PReLU(U)| @ |W|^T + |b|,  U32 = 2^-24, and
k_fwd_split = 16 * (longest slice in k-steps) + 2 + (KS - 1) + [bias] + [slope]  (that file derives it).  For K % 16 != 0 the call goes
to k_btlnk_fwd, whose k is k_fwd_direct of the same file.

Shapes: K = 80 (5 k-steps over 16 slices: empty slices, and one-step slices that only the tail runs), K = 272 (17 k-steps: an uneven
split), K = 64 * 204 once at B = 65 (51-step slices: twelve whole groups and a 3-step tail; rows past B in the second block);
B in {1, 63, 64, 65, 130}: a ragged last tile, more than one tile.  ops.btlnk_fwd's threshold between the two kernels is
BTLNK_SPLITK_MIN_B = 1, so no B lies below it: every B runs k_btlnk_fwd_t when K % 16 == 0, and K = 20 covers the other side of that
condition (k_btlnk_fwd)."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_refs import U32, dd
from test_gpu_btlnk_kernels import k_fwd_direct, k_fwd_split

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 130)
BMAX = max(BS)
SLOPE = 0.25


def _ref(d, a, bias):
    """double z [B, L] and M = sum |W| |PReLU(U)| + |b|"""
    U, W, b = dd(d["U"]), dd(d["W"]), dd(d["b"])
    X = U if a is None else torch.where(U > 0, U, R.f32(a) * U)
    z = X @ W.T + (b if bias else 0.0)
    M = X.abs() @ W.abs().T + (b.abs() if bias else 0.0)
    return z.numpy(), M.numpy()


def _check(d, K, L, Bs):
    from coskad_amd import _lib, ops
    KS = _lib.lib().coskad_btlnk_fwd_ks()
    dev = {k: v.cuda() for k, v in d.items()}
    worst = 0.0
    for a in (None, SLOPE):
        s = None if a is None else torch.tensor([a], dtype=torch.float32).cuda()
        for bias in (True, False):
            zr, M = _ref(d, a, bias)
            k = k_fwd_split(K, KS, a is not None, bias) if K % 16 == 0 else k_fwd_direct(K, a is not None, bias)
            for B in Bs:
                Ub = dev["U"][:B].contiguous()
                z = ops.btlnk_fwd(Ub, dev["W"], dev["b"] if bias else None, s)
                z2 = ops.btlnk_fwd(Ub, dev["W"], dev["b"] if bias else None, s)
                assert z.shape == (B, L)
                assert torch.equal(z.view(torch.int32), z2.view(torch.int32)), ("repeat", K, L, B, a, bias)
                err = np.abs(z.cpu().numpy().astype(np.float64) - zr[:B])
                bound = k * U32 * M[:B]
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (K, L, B, a, bias, ratio)
    print(f"RATIO btlnk_fwd K={K} L={L} {worst:.3f}")


@pytest.mark.parametrize("L", (8, 16))
@pytest.mark.parametrize("K", (80, 272, 20))
def test_btlnk_fwd_small(K, L):
    _check(R.btlnk_inputs(BMAX, K, L, seed=13 * K + L), K, L, BS)


def test_btlnk_fwd_headline_k():
    K, L, B = 64 * 204, 16, 65
    _check(R.btlnk_inputs(B, K, L, seed=5), K, L, (B,))

