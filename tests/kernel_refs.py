"""Float64 restatements of the stand-alone kernels the kernel-level tests compare with (test_gpu_wide_kernels.py,
test_gpu_narrow_conv.py, test_gpu_flat_kernels.py), in plain torch / numpy on the CPU.  Every function takes the float32 inputs
converted to double, composes the forward only -- gradients come from torch autograd on that forward, never from a hand-written
backward -- and never calls the library.  test_kernel_refs_host.py holds them against torch.nn / torch.optim before a device sees
them.  Not a conftest: a plain module the tests import by name."""
import math

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of float32 (round to nearest): one rounding moves a value x by at most U32 |x|
U64 = 2.0 ** -53


def f32(x):
    """the double a kernel sees when a Python float goes through a `float` parameter"""
    return float(np.float32(x))


def dd(t):
    return t.detach().double().cpu()


# ---- BatchNorm2d + residual + PReLU on [N, C, P] (csrc/wide.hip) -------------------------------------------------------------------------

def bn_batch_stats(x, eps):
    """x [N, C, P] double -> (mean [C], biased variance [C], invstd [C])"""
    mean = x.mean((0, 2))
    var = ((x - mean[None, :, None]) ** 2).mean((0, 2))
    return mean, var, 1.0 / torch.sqrt(var + eps)


def bn_running_update(mean, var, count, running_mean, running_var, momentum):
    """nn.BatchNorm2d's train-mode update: unbiased variance (count > 1), new = (1 - momentum) old + momentum batch"""
    unb = var * count / (count - 1.0) if count > 1 else var
    return (1.0 - momentum) * running_mean + momentum * mean, (1.0 - momentum) * running_var + momentum * unb


def bn_affine(x, gamma, beta, eps, training, running_mean=None, running_var=None):
    """BatchNorm2d's output on x [N, C, P]: batch statistics (differentiated through) in training mode, the running ones otherwise.
    -> (y, mean, invstd)"""
    if training:
        mean, _, inv = bn_batch_stats(x, eps)
    else:
        mean, inv = running_mean, 1.0 / torch.sqrt(running_var + eps)
    y = (x - mean[None, :, None]) * (inv * gamma)[None, :, None] + beta[None, :, None]
    return y, mean, inv


def prelu(u, a):
    return torch.where(u > 0, u, a * u)


def bn2_block(Ct, Cr, t, r, slope, eps, training, mask=None):
    """out = PReLU(mask * BN_t(Ct) + BN_r(Cr)); t / r: dicts gamma, beta (+ running_mean, running_var in eval mode); r None: identity
    residual.  -> (out, u, (mean_t, inv_t), (mean_r, inv_r) or None)"""
    yt, mt, it = bn_affine(Ct, t["gamma"], t["beta"], eps, training, t.get("running_mean"), t.get("running_var"))
    if mask is not None:
        yt = mask * yt
    if r is None:
        yr, sr = Cr, None
    else:
        yr, mr, ir = bn_affine(Cr, r["gamma"], r["beta"], eps, training, r.get("running_mean"), r.get("running_var"))
        sr = (mr, ir)
    u = yt + yr
    return prelu(u, slope), u, (mt, it), sr


# ---- the dropout hash of wide::drop_mask --------------------------------------------------------------------------------------------------

M64 = (1 << 64) - 1


def drop_hash24(seed, i):
    """the 24 bits wide::drop_mask compares with p, in Python integers masked to 64 bits"""
    x = (i * 0x9E3779B97F4A7C15 + seed) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 40


def drop_mask_twin(n, p, seed):
    """float32 [n]: 0 or 1 / (1 - p), the kernel's value for element i (p == 0: ones).  u = h / 2^24 is exact in float32, so u >= p
    is h >= p 2^24 with p the float32 the kernel receives."""
    if p == 0.0:
        return np.ones(n, np.float32)
    p32 = np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    thr = float(p32) * 16777216.0
    return np.array([scale if drop_hash24(seed, i) >= thr else 0.0 for i in range(n)], np.float32)


def drop_mask_twin_np(n, p, seed):
    """drop_mask_twin on numpy uint64 arrays (whose arithmetic wraps at 64 bits), for tensors too large for a Python loop;
    test_kernel_refs_host.py holds the two equal"""
    if p == 0.0:
        return np.ones(n, np.float32)
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    p32 = np.float32(p)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    keep = (x >> np.uint64(40)).astype(np.float64) >= float(p32) * 16777216.0
    return np.where(keep, scale, np.float32(0.0)).astype(np.float32)


DROP_SEEDS = (12345, (1 << 40) + 17)       # test_gpu_wide_kernels.test_dropout_mask_is_the_restated_hash: one above 2^32


def bn2_case_seed(Nb, C, P, residual_bn, training, drop_p):
    """the data seed of one apply / backward case (its dropout seed is (1 << 33) + this)"""
    return 1000 * Nb + 10 * C + P + int(residual_bn) + 2 * int(training) + int(drop_p * 100)


# ---- narrow convolution (csrc/last_layer.hip) ---------------------------------------------------------------------------------------------

def narrow_conv(U, slope, W):
    """[B, Ci, TV] x [J, Ci] -> [B, J, TV]: W . PReLU(U) (slope None: U is activated already)"""
    X = U if slope is None else prelu(U, slope)
    return torch.einsum("jc,bcp->bjp", W, X)


# ---- reconstruction head (csrc/stsgcn_fwd.hip) -------------------------------------------------------------------------------------------

def rec_head(U, x, slope):
    """mean((PReLU(U) - x)^2)"""
    return ((prelu(U, slope) - x) ** 2).mean()


# ---- Adam (csrc/heads.hip) ----------------------------------------------------------------------------------------------------------------

def adam_step(p, g, m, v, t, lr, beta1, beta2, eps, mask=None, gscale=1.0, reg_coef=0.0):
    """torch.optim.Adam's step t (1-based; amsgrad off, weight_decay 0) on double arrays with the regulariser's gradient folded in:
    g' = g gscale + reg_coef mask p.  -> (p, m, v)"""
    g = g * gscale + reg_coef * (mask if mask is not None else 1.0) * p
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


# ---- gather + affine transform (csrc/data.hip) -------------------------------------------------------------------------------------------

def gather_transform_f32(xy, mats, index, N, ntrans):
    """float32, in the kernel's order (x m0 + y m1) + m2 with every operation rounded (numpy never contracts to an FMA); an index
    below 0 or with index // N >= ntrans gives a zero clip.  xy [N, 2, TV], mats [ntrans, 3, 3] -> [B, 2, TV]"""
    out = np.zeros((len(index), 2, xy.shape[2]), np.float32)
    for b, i in enumerate(index):
        i = int(i)
        if i < 0 or i // N >= ntrans:
            continue
        s, t = i % N, i // N
        x, y, m = xy[s, 0], xy[s, 1], mats[t]
        out[b, 0] = (x * m[0, 0] + y * m[0, 1]) + m[0, 2]
        out[b, 1] = (x * m[1, 0] + y * m[1, 1]) + m[1, 2]
    return out
