"""Float64 restatements of the stand-alone kernels the kernel-level tests compare with (test_gpu_wide_kernels.py,
test_gpu_narrow_conv.py, test_gpu_flat_kernels.py, test_gpu_head_kernels.py, test_gpu_btlnk_kernels.py, test_gpu_decoder_kernels.py),
in plain torch / numpy on the CPU (the PowerSpherical restatement at the end, shared by test_gpu_ae_step.py and
test_gpu_ae_wide_latent.py, builds on the package's torch distribution class, not on a kernel).  Every function takes
the float32 inputs converted to double, composes the forward only -- gradients come from torch autograd on that forward, never from a
hand-written backward -- and never calls the library.  test_kernel_refs_host.py holds them against torch.nn / torch.optim before a
device sees them.  The one-class heads' section also restates the kernels' Poincare sequences, backward included, over a running-error
arithmetic: that restatement supplies BOUNDS only, the values compared with stay the oracle's.  Not a conftest: a plain module the
tests import by name."""
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


# ---- the one-class heads (csrc/heads.hip over the maps of latent_row.h: L <= 16 one thread per clip, 16 < L <= 512 one wave per clip) --

HEAD_LMAX = 16            # latent_row.h LMAX: latents up to here run one thread per clip
HEAD_ROWS = 512           # kFlatBlock: clips per block of the narrow heads; one block writes stats / acc itself
WIDE_TILE = 16            # kWideTileRows (heads_common.h): clips per block of the wide heads (4 waves)
WIDE_MAX_BLOCKS = 1024    # kWideMaxBlocks

# Largest error of the device's tanhf / log1pf in ulps of the float32 result.  Neither can be derived from the kernels' text; both were
# measured once on an MI355X (torch's float32 tanh / log1p on the device against float64 over the argument ranges of
# head_inputs: 1.39 and 0.57 ulp) and set to the ceiling of the largest error seen plus 1 ulp.
TANH_ULP = 3
LOG1P_ULP = 2

HEAD_RADII = (0.0, 1e-7, 9e-6, 1.1e-5, 1e-3, 0.3, 1.0, 2.5, 3.7, 3.9, 6.0, 14.9, 15.1, 20.0, 100.0)
HEAD_CENTRES = (0.0, 0.4, 0.93, 0.995)


def head_inputs(B, L, cnorm, seed=0):
    """Latent rows and a centre for the head tests: row n is a random unit direction times HEAD_RADII[(n + seed) % 15] -- the radii
    straddle the min-norm clamp (1e-5), the projection threshold artanh(0.999) = 3.8002 and the tanh clamp (15) -- and, for a centre off
    the origin, row 0 is antipodal to it at radius 6 and row 1 lies along it at radius 1 (B == 1: one of the two, by the seed).
    -> (z [B, L] float32, c [L] float32 with |c| = cnorm)"""
    g = torch.Generator().manual_seed(1000 * L + 7 * B + seed)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    cdir = unit(torch.randn(L, generator=g, dtype=torch.float64))
    dirs = unit(torch.randn(B, L, generator=g, dtype=torch.float64))
    radii = torch.tensor(HEAD_RADII, dtype=torch.float64)[(torch.arange(B) + seed) % len(HEAD_RADII)]
    z = dirs * radii[:, None]
    if cnorm > 0:
        special = [-6.0 * cdir, 1.0 * cdir]
        if B == 1:
            z[0] = special[seed % 2]
        else:
            z[0], z[1] = special
    return z.float(), (cnorm * cdir).float()


def dot_roundings(L):
    """roundings of one latent dot product: the fmaf chain of the L non-zero products (narrow), or the lane's ceil(L / 64) fmaf and the
    six xor-butterfly levels of wave_sum (wide)"""
    return L if L <= HEAD_LMAX else -(-L // 64) + 6


def head_blocks(B, L):
    """partial rows (= blocks) of a head launch"""
    if L <= HEAD_LMAX:
        return 1 if B <= HEAD_ROWS else -(-B // HEAD_ROWS)
    return min(-(-B // WIDE_TILE), WIDE_MAX_BLOCKS)


def head_sum_roundings(B, L):
    """float32 roundings on the way from a clip's term to its slot of `stats`, the final conversion included (the partial rows are
    summed in double).  Narrow: the thread's clips in turn, wave_sum (6), the block's eight waves in turn (7; the first add is to 0),
    the conversion (1).  Wide (Euclidean / Poincare): the wave's clips in turn, the four waves (3), the conversion (1)."""
    P = head_blocks(B, L)
    if L <= HEAD_LMAX:
        return -(-B // (P * HEAD_ROWS)) + 6 + 7 + 1
    return -(-B // (P * 4)) + 3 + 1


def poincare_slot_sums(zh):
    """the Poincare head's slots from the points on the ball: (sum gamma zh [L], sum (gamma - 1), sum |zh|), gamma = 2 / (1 - |zh|^2)"""
    gamma = 2.0 / (1.0 - (zh * zh).sum(-1, keepdim=True))
    return (gamma * zh).sum(0), (gamma - 1.0).sum(), torch.sqrt((zh * zh).sum(-1)).sum()


def euclid_slot_sums(z):
    """the Euclidean / Mahalanobis heads' slots: (sum z [L], the clip count, sum |z|) and the Gram matrix sum z z^T"""
    return z.sum(0), float(z.shape[0]), torch.sqrt((z * z).sum(-1)).sum(), z.T @ z


def midpoint_from_sums(S, s):
    """oracle.ref_cpu.weighted_midpoint from its two sums S = sum gamma x, s = sum (gamma - 1) (curvature 1), line for line"""
    m = S / s.clamp_min(1e-10)
    mn = torch.sqrt((m * m).sum()).clamp_min(1e-15)
    at = 0.5 * torch.log((1 + mn.clamp(max=1 - 1e-7)) / (1 - mn.clamp(max=1 - 1e-7)))
    return torch.tanh(0.5 * at) * m / mn


# Running-error arithmetic: the kernels' Poincare chain (expmap0 -> project -> Mobius add -> artanh, and its backward) is too long and
# too ill-conditioned for a hand constant, so its BOUND comes from restating the kernels' operation sequence once (the functions
# below) over a value / error pair: EV.v is the operation on the exact operands in double, EV.e bounds how far the kernel's float32
# value can be from it -- every operation propagates its operands' errors (sum |df/dx_i| e_i, with the denominators taken at their
# near end) and adds one float32 rounding of its result, U32 (|v| + e).  The VALUE the tests compare with stays the oracle's; the
# restatement in double is held to the oracle at 1e-12 and, evaluated over F32 (numpy float32, every operation rounded), to its own
# bound by test_kernel_refs_host.py.

def _pow2(x):
    return x == 0.0 or math.frexp(abs(x))[0] == 0.5


class EV:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=torch.float64) + torch.zeros_like(self.v)

    @staticmethod
    def lift(x):
        if isinstance(x, EV):
            return x
        assert f32(x) == x, "a literal must be a float32"
        return EV(x)

    @staticmethod
    def rounded(v, ep):
        return EV(v, ep + U32 * (v.abs() + ep))

    def __neg__(self):
        return EV(-self.v, self.e)

    def __add__(self, o):
        o = EV.lift(o)
        return EV.rounded(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-EV.lift(o))

    def __rsub__(self, o):
        return EV.lift(o) + (-self)

    def __mul__(self, o):
        if not isinstance(o, EV) and _pow2(o):
            return EV(self.v * o, self.e * abs(o))          # exact
        o = EV.lift(o)
        return EV.rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = EV.lift(o)
        v = self.v / o.v
        return EV.rounded(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e).clamp_min(1e-300))

    def __rtruediv__(self, o):
        return EV.lift(o) / self

    def sqrt(self):
        v = torch.sqrt(self.v)
        lo = torch.sqrt((self.v - self.e).clamp_min(0.0))
        ep = torch.where(self.e > 0, torch.minimum(self.e / (v + lo).clamp_min(1e-300), torch.sqrt(self.e)), torch.zeros_like(v))
        return EV.rounded(v, ep)

    def tanh(self):
        v = torch.tanh(self.v)
        near = torch.tanh((self.v.abs() - self.e).clamp_min(0.0))
        return EV(v, (1.0 - near * near) * self.e + TANH_ULP * 2 * U32 * v.abs())

    def log1p(self):
        v = torch.log1p(self.v)
        return EV(v, self.e / (1.0 + self.v - self.e).clamp_min(1e-300) + LOG1P_ULP * 2 * U32 * v.abs())

    def _pick(self, o, v):
        """min / max are 1-Lipschitz: the larger of the two errors, and the winner's own where the two cannot change places"""
        o = EV.lift(o)
        z = torch.zeros_like(self.v)
        ov, oe = o.v + z, o.e + z
        apart = (self.v - ov).abs() > self.e + oe
        return EV(v(self.v, ov), torch.where(apart, torch.where(v(self.v, ov) == self.v, self.e, oe), torch.maximum(self.e, oe)))

    def maximum(self, o):
        return self._pick(o, torch.maximum)

    def minimum(self, o):
        return self._pick(o, torch.minimum)


class EVMath:
    """the arithmetic the chains are written over: constants, selects, the latent dot product and the record of every select's margin"""

    def __init__(self):
        self.margins = []          # (name, |x - threshold| [rows], err(x) + err(threshold) [rows])

    def inp(self, x):
        return EV(torch.as_tensor(np.asarray(x), dtype=torch.float64) if not torch.is_tensor(x) else x.double())

    def const(self, x, x32=None):
        """a constant the kernel holds as float32: x32 (default: x rounded) where the exact chain has x"""
        return EV(x, abs((f32(x) if x32 is None else float(x32)) - x))

    def exact(self, x):
        """x taken as an exact operand: for a result that does not depend on x's value"""
        return EV(x.v)

    def rel(self, x):
        return x.e / (x.v.abs() - x.e).clamp_min(1e-300)

    def widen(self, x, rel):
        return EV(x.v, x.e + rel * (x.v.abs() + x.e))

    def gt(self, name, x, thr):
        thr = EV.lift(thr)
        self.margins.append((name, (x.v - thr.v).abs(), x.e + thr.e))
        return x.v > thr.v

    def positive(self, x):
        return x.v > 0

    def where(self, cond, a, b):
        a, b = EV.lift(a), EV.lift(b)
        return EV(torch.where(cond, a.v, b.v + torch.zeros_like(a.v)), torch.where(cond, a.e, b.e + torch.zeros_like(a.e)))

    def dot(self, a, b, wide):
        """[.., L] x [.., L] -> [.., 1] in the kernel's order: dot() of latent_row.h, one fmaf chain (PerThread) or, wide, lane l's chain over
        j = l + 64 i, then wave_sum (PerWave).  Every partial sum is rounded once."""
        t = a.v * b.v
        prop = (a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e).sum(-1, keepdim=True)
        L = t.shape[-1]
        if not wide:
            run = t.cumsum(-1).abs().sum(-1, keepdim=True)
            n = L
        else:
            pad = torch.zeros(t.shape[:-1] + (512 - L,), dtype=t.dtype)
            lanes = torch.cat([t, pad], -1).view(t.shape[:-1] + (8, 64))
            nv = -(-L // 64)
            run = lanes.cumsum(-2)[..., :nv, :].abs().sum((-2, -1)).unsqueeze(-1) + 6 * t.abs().sum(-1, keepdim=True)
            n = nv + 6
        return EV(t.sum(-1, keepdim=True), prop + U32 * (run + n * prop))

    def value(self, x):
        return x.v

    def bound(self, x):
        return x.e


class F32:
    """numpy float32 with the same interface: every operation rounds to float32 (an fmaf is formed in double and rounded once)"""
    __slots__ = ("x",)

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float32)

    @staticmethod
    def lift(o):
        return o if isinstance(o, F32) else F32(np.float32(o))

    def __neg__(self):
        return F32(-self.x)

    def __add__(self, o):
        return F32(self.x + F32.lift(o).x)

    __radd__ = __add__

    def __sub__(self, o):
        return F32(self.x - F32.lift(o).x)

    def __rsub__(self, o):
        return F32(F32.lift(o).x - self.x)

    def __mul__(self, o):
        return F32(self.x * F32.lift(o).x)

    __rmul__ = __mul__

    def __truediv__(self, o):
        with np.errstate(divide="ignore", invalid="ignore"):
            return F32(self.x / F32.lift(o).x)

    def __rtruediv__(self, o):
        return F32.lift(o) / self

    def sqrt(self):
        return F32(np.sqrt(self.x))

    def tanh(self):
        return F32(np.tanh(self.x.astype(np.float64)))

    def log1p(self):
        return F32(np.log1p(self.x.astype(np.float64)))

    def maximum(self, o):
        return F32(np.maximum(self.x, F32.lift(o).x))

    def minimum(self, o):
        return F32(np.minimum(self.x, F32.lift(o).x))


class F32Math:
    def __init__(self):
        self.margins = []

    def inp(self, x):
        return F32(x.numpy() if torch.is_tensor(x) else x)

    def const(self, x, x32=None):
        return F32(np.float32(x if x32 is None else x32))

    def exact(self, x):
        return x

    def rel(self, x):
        return None

    def widen(self, x, rel):
        return x

    def gt(self, name, x, thr):
        return x.x > F32.lift(thr).x

    def positive(self, x):
        return x.x > 0

    def where(self, cond, a, b):
        return F32(np.where(cond, F32.lift(a).x, F32.lift(b).x))

    @staticmethod
    def _fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)

    def dot(self, a, b, wide):
        a, b = np.broadcast_arrays(a.x, b.x)
        L = a.shape[-1]
        if not wide:
            s = np.zeros(a.shape[:-1], np.float32)
            for j in range(L):
                s = self._fma(a[..., j], b[..., j], s)
            return F32(s[..., None])
        pad = [(0, 0)] * (a.ndim - 1) + [(0, 512 - L)]
        a, b = (np.pad(t, pad).reshape(t.shape[:-1] + (8, 64)) for t in (a, b))
        s = np.zeros(a.shape[:-2] + (64,), np.float32)
        for v in range(8):
            s = self._fma(a[..., v, :], b[..., v, :], s)
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[..., lane ^ off]
        return F32(s[..., :1])

    def value(self, x):
        return torch.from_numpy(x.x.astype(np.float64))


def _f32sub(a, b):
    return float(np.float32(a) - np.float32(b))


def hyp_embed(A, u, wide):
    """heads.hip hyp_embed<M>: p = project(expmap0(u)) and what the backward keeps"""
    kmin = A.const(1e-5)
    un_raw = A.dot(u, u, wide).sqrt()
    un = un_raw.maximum(kmin)
    tn = un.minimum(15.0).tanh()                                  # the lower clamp at -15 never binds
    f = tn / un
    e = f * u
    en_raw = A.dot(e, e, wide).sqrt()
    en = en_raw.maximum(kmin)
    maxnorm = A.const(1 - 1e-3, _f32sub(1, 1e-3))
    clamped = A.gt("projection", en, maxnorm)
    # x / |x| does not change when x is scaled, so the projected point carries none of f's error: only the roundings from e on
    e0 = A.exact(f) * u
    p = A.where(clamped, e0 / A.dot(e0, e0, wide).sqrt().maximum(kmin) * maxnorm, e)
    return dict(p=p, un_raw=un_raw, un=un, tn=tn, f=f, en_raw=en_raw, clamped=clamped, maxnorm=maxnorm, kmin=kmin)


def poincare_dist(A, c, p, wide, need_grad=True):
    """poincare_dist of both files: d = 2 artanh(|(-c) (+) p|) [.., 1] and dd/dp.  The artanh clamp is a minimum, continuous, and the
    backward takes the clamped value on both sides of it (Artanh.backward): its error propagates without a select."""
    x2, y2, xy = A.dot(c, c, wide), A.dot(p, p, wide), -A.dot(c, p, wide)
    alpha = 1.0 + 2.0 * xy + y2
    beta = 1.0 - x2
    den = 1.0 + 2.0 * xy + x2 * y2
    D = den + A.const(1e-5)
    x = -c
    m = (alpha * x + beta * p) / D
    mn = A.dot(m, m, wide).sqrt()
    mc = mn.minimum(A.const(1 - 1e-5, _f32sub(1, 1e-5)))          # the lower clamp never binds: mn >= 0
    d = mc.log1p() - (-mc).log1p()
    if not need_grad:
        return d, None, None
    # everything from here to dz is linear in gmn = 2 / (1 - mc^2), the one badly conditioned scalar (1 / (1 - mc^2) reaches 5e4): its
    # relative error goes to dz as a relative error (hyp_embed_bwd's caller widens by it), not through the cancellations on the way
    gmn = 2.0 / (1.0 - mc * mc)
    rel = A.rel(gmn)
    gmn = A.exact(gmn)
    inv = A.where(A.positive(mn), gmn / mn, 0.0)
    gm = inv * m
    gD = -A.dot(gm, m, wide) / D
    galpha = A.dot(gm / D, x, wide)
    gp = beta * gm / D + galpha * (2.0 * x + 2.0 * p) + gD * (2.0 * x + 2.0 * x2 * p)
    return d, gp, rel


def hyp_embed_bwd(A, u, em, gp, wide):
    """hyp_embed_bwd of both files: dL/dp -> dL/du through project and expmap0"""
    f, un, tn = em["f"], em["un"], em["tn"]
    en = em["en_raw"]
    egp = A.dot(f * u, gp, wide)
    ge = A.where(em["clamped"], em["maxnorm"] * (gp / en - f * u * egp / (en * en * en)), gp)
    gf = A.dot(ge, u, wide)
    sech2 = A.where(A.gt("tanh clamp", A.const(15.0), un), 1.0 - tn * tn, 0.0)
    df = (sech2 * un - tn) / (un * un)
    coef = A.where(A.gt("min-norm", em["un_raw"], em["kmin"]), gf * df / em["un_raw"], 0.0)
    return f * ge + coef * u


def poincare_head_chain(A, z, c, wide, gscale=None):
    """one clip of k_poincare_head<M> on float32 z [B, L], c [L] or None: zh, the slot terms gamma zh, gamma - 1,
    |zh|, and with a centre the distance and dz = hyp_embed_bwd(gscale dd/dp) (gscale: (exact, as the kernel's float32 holds it))"""
    u = A.inp(z)
    em = hyp_embed(A, u, wide)
    p = em["p"]
    y2 = A.dot(p, p, wide)
    gamma = 2.0 / (1.0 - y2)
    out = dict(zh=p, gzh=gamma * p, gm1=gamma - 1.0, norm=y2.sqrt())
    if c is not None:
        d, gp, rel = poincare_dist(A, _row(A, c), p, wide, gscale is not None)
        out["d"] = d
        if gscale is not None:
            out["dz"] = A.widen(hyp_embed_bwd(A, u, em, gp * A.const(*gscale), wide), rel)
    return out


def _row(A, c):
    x = A.inp(c)
    if isinstance(x, EV):
        return EV(x.v[None, :], x.e[None, :])
    return F32(x.x[None, :])


def logmap0_chain(A, y, wide):
    """k_poincare_logmap0 of both files"""
    p = A.inp(y)
    yn = A.dot(p, p, wide).sqrt().maximum(A.const(1e-5))
    yc = yn.minimum(A.const(1 - 1e-5, _f32sub(1, 1e-5)))
    at = 0.5 * (yc.log1p() - (-yc).log1p())
    return p / yn * at


def gscale_pair(upstream, B):
    """the Poincare / Mahalanobis heads' gscale = upstream / (float)B: (exact on the float32 upstream, the kernel's float32)"""
    up = np.float32(upstream)
    return float(up) / B, float(up / np.float32(B))


# ---- the bottleneck projection (csrc/bottleneck.hip: L <= 16; csrc/btlnk_chain.hip; csrc/btlnk_wide.hip: 16 < L <= 512) ------------------

def btlnk(U, slope, W, b):
    """z = W . PReLU(U) + b on U [B, K], W [L, K], b [L] or None (slope None: U is activated already)"""
    X = U if slope is None else prelu(U, slope)
    z = X @ W.T
    return z if b is None else z + b


def top_layer_sums(dU, Z, x_in, in_slope):
    """the batch reductions the top layer's BatchNorm backward starts from (coskad_hip.h, coskad_btlnk_bwd_chain_f32):
    P[o][c] = sum dU[n][o][p] Z[n][c][p], Q[o][c] = sum dU[n][o][p] PReLU(x_in)[n][c][p], s[o] = sum dU[n][o][p];
    dU [B, Co, TV], Z / x_in [B, Ci, TV] -> (P [Co, Ci], Q [Co, Ci], s [Co])"""
    X = x_in if in_slope is None else prelu(x_in, in_slope)
    return torch.einsum("nop,ncp->oc", dU, Z), torch.einsum("nop,ncp->oc", dU, X), dU.sum((0, 2))


BTLNK_MAGS = (1e-3, 1.0, 30.0)
F32_TINY = 2.0 ** -126


def btlnk_zero_plants(B, K, TV=None):
    """(clip, column) of the exact zeros btlnk_inputs plants, signs alternating +0.0, -0.0 in this order: the first, second, middle
    and last element of U; and in the last clip of every 16-clip tile one element at column (5 + 7 tile) % K and one inside the last
    position tile (K = channels x TV positions, position innermost; TV None: one channel of K positions).  At most a quarter of U
    (one element of a U below eight) is planted, the head of this order."""
    TV = K if TV is None else TV
    n = B * K
    flat = [0, 1, n // 2, n - 1] if n > 1 else [0]
    spots = [(e // K, e % K) for e in flat]
    p_last = 16 * ((TV - 1) // 16)
    for t in range(-(-B // 16)):
        row = min(16 * t + 15, B - 1)
        spots.append((row, (5 + 7 * t) % K))
        ch = t % (K // TV)
        spots.append((row, ch * TV + p_last + t % (TV - p_last)))
    seen, out = set(), []
    for s in spots:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out[:max(1, n // 4)]          # (a U of three or four elements keeps the others: at most a quarter is zero)


def btlnk_inputs(B, K, L, seed, TV=None):
    """float32 inputs of the bottleneck tests: U [B, K] a normal draw times a per-element magnitude from BTLNK_MAGS with exact +0.0 /
    -0.0 at btlnk_zero_plants; W ~ N(0, 1 / K) [L, K]; b, dz ~ N(0, 1).  No value is subnormal (how the f32 MFMA treats subnormals is
    not documented)."""
    g = torch.Generator().manual_seed(seed)
    mags = torch.tensor(BTLNK_MAGS)[torch.randint(0, len(BTLNK_MAGS), (B, K), generator=g)]
    U = (torch.randn(B, K, generator=g) * mags).contiguous()
    for i, (n, k) in enumerate(btlnk_zero_plants(B, K, TV)):
        U[n, k] = -0.0 if i % 2 else 0.0
    d = dict(U=U, W=torch.randn(L, K, generator=g) * K ** -0.5, b=torch.randn(L, generator=g), dz=torch.randn(B, L, generator=g))
    for k, v in d.items():
        assert not bool(((v != 0) & (v.abs() < F32_TINY)).any()), f"subnormal in {k}"
    return d


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


# Restatements of the launch plans: they size the bounds (chain lengths) and prove that a test shape meets the edge it is listed for;
# test_kernel_refs_host.py holds each against what the library reports through its workspace / row queries.

def btl_chunks(B, K):
    """csrc/bottleneck.hip btl_chunks with coskad_btlnk_bwd_f32's chunk length -> (S clip chunks, clips per chunk)"""
    gx = ceil_div(K, 256)
    s = max(1, min((1024 + gx // 2) // gx, ceil_div(B, 16), 64))
    return s, round_up(ceil_div(B, s), 16)


def btl_bwd_ws_floats(B, K, L):
    S, _ = btl_chunks(B, K)
    return S * L * K + S * ceil_div(K, 256) + 64


def chain_plan(B, TV):
    """csrc/btlnk_chain.hip bc::plan -> (position tiles, S clip chunks, clips per chunk); rows = position tiles x S"""
    npt = ceil_div(TV, 16)
    s = max(1, min(256 // npt, ceil_div(B, 16)))
    chunk = round_up(ceil_div(B, s), 16)
    return npt, ceil_div(B, chunk), chunk


def chain_floats(B, TV, Ci, Co=64):
    npt, S, _ = chain_plan(B, TV)
    E = 2 * Co * Ci + Co
    return (npt * S * E + 1) // 2 * 2 + 2 * E


def wide_tile(L):
    """bw::fwd_tn / bw::dw_tm: 16-wide MFMA tiles per wave along the latent axis"""
    return 1 if L <= 32 else (2 if L <= 64 else 4)


def wide_fwd_rchunk(K, L):
    ks = max(2, 16 // ceil_div(L, 32 * wide_tile(L)))
    ks = max(1, min(ks, ceil_div(K, 8 * 16)))
    return round_up(ceil_div(K, ks), 16)


def wide_fwd_slices(K, L):
    return ceil_div(K, wide_fwd_rchunk(K, L))


def wide_dw_chunk(B, K, L):
    tiles = ceil_div(K, 128) * ceil_div(L, 32 * wide_tile(L))
    s = max(1, min((1024 + tiles // 2) // tiles, 64))
    return round_up(ceil_div(B, s), 16)


def wide_dw_chunks(B, K, L):
    return ceil_div(B, wide_dw_chunk(B, K, L))


def wide_dx_blocks(B, K):
    return ceil_div(K, 128) * ceil_div(B, 128)


# ---- the decoder models' stand-alone kernels (test_gpu_decoder_kernels.py) ----------------------------------------------------------------
# rev_btlnk at latent 8 / 16 (csrc/rev_btlnk.hip)

def rev_btlnk(z, W, b):
    """H = z W^T + b on z [B, L], W [N, L], b [N] or None (nn.Linear(latent -> hidden T V), ae.py:223-227)"""
    H = z @ W.T
    return H if b is None else H + b


def rev_slices(B, N):
    """csrc/rev_btlnk.hip rb::slices: clip slices of the backward's (column blocks) x (slices) grids"""
    if B < 16:
        return 1
    s = ceil_div(1024, ceil_div(N // 4, 256))
    s = min(max(s, 16), 64, B // 16)
    return max(s, 1)


def rev_fwd_slices(B, N):
    """coskad_rev_btlnk_fwd_f32's three branches"""
    return 1 if B < 64 else (4 if B < 1024 else rev_slices(B, N))


def rev_inputs(B, N, L, seed):
    """float32 inputs of the rev_btlnk tests: z ~ N(0, 1) with a per-clip magnitude from BTLNK_MAGS, W ~ N(0, 1 / L) with a per-column
    offset (a zero-mean W would hide a dropped clip in db less than in dW), bias, dH ~ N(0, 1), a prior for dz"""
    g = torch.Generator().manual_seed(seed)
    mags = torch.tensor(BTLNK_MAGS)[torch.randint(0, len(BTLNK_MAGS), (B, 1), generator=g)]
    d = dict(z=(torch.randn(B, L, generator=g) * mags).contiguous(), W=torch.randn(N, L, generator=g) * L ** -0.5 + 0.1,
             b=torch.randn(N, generator=g), dH=torch.randn(B, N, generator=g) + 0.25, dz0=torch.randn(B, L, generator=g))
    for k, v in d.items():
        assert not bool(((v != 0) & (v.abs() < F32_TINY)).any()), f"subnormal in {k}"
    return d


# the folded first decoder layer's statistics algebra (csrc/lowrank_fold.hip, coskad_amd/lowrank.py)

FOLD_K = 9                # latent 8 + the constant image
FOLD_ROUND = 256          # positions per round (kThreads); MAXPOS = 2 rounds


def fold(X, G, gammas, betas, eps, n_pos):
    """The fold algebra in double.  X [2, 9, Co, TV] (branch r's rank-9 tensor), G [9, 9] or [Co, 9, 9] (a copy per channel: its
    gradient is then the per-channel share), gammas / betas: two [Co] tensors, eps: two floats.
        xbar[r, l, c] = sum_p X,   xx[r, c, l, m] = sum_p X_l X_m,
        mean = sum_l G[l, 8] xbar_l / n_pos,   E2 = sum_lm G[l, m] xx[l, m] / n_pos,   var = max(E2 - mean^2, 0),
        a = gamma / sqrt(var + eps),   Mw[c, p, l] = sum_r a_r X_rl (l < 8),   Mb[c, p] = sum_r a_r X_r8 + sum_r (beta_r - a_r mean_r).
    The clamp is there for rounding only (the true variance is never negative) and the operation folded, nn.BatchNorm2d, differentiates
    through its variance at 0 too: the clamp passes the gradient straight through.  -> dict"""
    Co = X.shape[2]
    Gc = G if G.dim() == 3 else G[None].expand(Co, FOLD_K, FOLD_K)
    xbar = X.sum(-1)                                                # [2, 9, Co]
    xx = torch.einsum("rlcp,rmcp->rclm", X, X)                      # [2, Co, 9, 9]
    mean = torch.einsum("cl,rlc->rc", Gc[:, :, FOLD_K - 1], xbar) / n_pos
    E2 = torch.einsum("clm,rclm->rc", Gc, xx) / n_pos
    raw = E2 - mean * mean
    var = raw + (raw.clamp(min=0.0) - raw).detach()
    epsv = torch.tensor([f32(eps[0]), f32(eps[1])], dtype=torch.float64)[:, None]
    istd = 1.0 / torch.sqrt(var + epsv)
    gam, bet = torch.stack(list(gammas)), torch.stack(list(betas))
    a = gam * istd
    M = torch.einsum("rc,rlcp->cpl", a, X)
    Mb = M[:, :, FOLD_K - 1] + (bet - a * mean).sum(0)[:, None]
    return dict(xbar=xbar, xx=xx, mean=mean, E2=E2, var=var, istd=istd, a=a, Mw=M[:, :, :FOLD_K - 1], Mb=Mb)


def fold_running(mean, var, n_pos, cbias, rmean, rvar, momentum):
    """nn.BatchNorm2d's update of one branch behind a conv with bias `cbias` (None: none): the bias shifts the mean only"""
    mom = f32(momentum)
    unb = n_pos / (n_pos - 1.0) if n_pos > 1 else 1.0
    mb = mean if cbias is None else mean + cbias
    return (1.0 - mom) * rmean + mom * mb, (1.0 - mom) * rvar + mom * var * unb


def fold_inputs(Co, TV, n, seed):
    """float32 / float64 inputs of the fold tests: latents zt = [z, 1] of n clips and G = zt^T zt (symmetric bit for bit), n_pos = n TV;
    X with a per-image scale; channel 1 (where there is one) has branch 0 all zero -- variance exactly 0 -- and the last channel of
    Co >= 3 a constant image 10^3 times the others' spread."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, FOLD_K - 1, generator=g, dtype=torch.float64) * 0.7 + 0.2
    zt = torch.cat([z, torch.ones(n, 1, dtype=torch.float64)], 1)
    G = zt.T @ zt
    G = 0.5 * (G + G.T)
    X = torch.randn(2, FOLD_K, Co, TV, generator=g) * torch.linspace(0.3, 1.5, FOLD_K)[None, :, None, None]
    if Co >= 2:
        X[0, :, 1] = 0.0
    if Co >= 3:
        X[:, FOLD_K - 1, Co - 1] = X[:, FOLD_K - 1, Co - 1] * 0.5 + 2000.0       # (the expanded layer's spread there is about 2)
    d = dict(X=X.contiguous(), G=G, zt=zt, n_pos=float(n * TV))
    for r in range(2):
        d[f"gamma{r}"] = torch.rand(Co, generator=g) + 0.5
        d[f"beta{r}"] = torch.randn(Co, generator=g)
        d[f"cbias{r}"] = torch.randn(Co, generator=g)
        d[f"rmean{r}"] = torch.randn(Co, generator=g)
        d[f"rvar{r}"] = torch.rand(Co, generator=g) + 0.5
    d["dMw"] = torch.randn(Co * TV, FOLD_K - 1, generator=g)
    d["dMb"] = torch.randn(Co * TV, generator=g) + 0.3
    return d


# the `mlp` projector's tail (csrc/mlp_head.hip)

MLP_HP = 16               # hidden, out <= 16: the 64-rows-per-block kernels
MLP_RB = 64


def mlp_fast(H, L):
    return H <= MLP_HP and L <= MLP_HP


def mlp_head(y, gamma, beta, W2, b2, eps, training, running_mean=None, running_var=None):
    """z = W2 relu(BatchNorm1d(y)) + b2 in double on y [B, H]: batch statistics (biased variance, differentiated through) in training
    mode, the running ones otherwise.  -> dict z, y2, xh, mean, var, inv"""
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
    else:
        mean, var = running_mean, running_var
    inv = 1.0 / torch.sqrt(var + f32(eps))
    xh = (y - mean) * inv
    y2 = xh * gamma + beta
    z = torch.relu(y2) @ W2.T
    if b2 is not None:
        z = z + b2
    return dict(z=z, y2=y2, xh=xh, mean=mean, var=var, inv=inv)


MLP_PLANTS = 5            # from this many features on, features 1 .. 4 are planted


def mlp_inputs(B, H, L, seed):
    """float32 inputs of the mlp_head tests.  y ~ N(offset_k, scale_k^2) per feature; with H >= 5: feature 1 has gamma = beta = 0 (gate
    closed, exactly), feature 2 gamma = 0, beta = 0.75 (gate open everywhere), feature 3 is the constant 1.5 (sums of 1.5 and 2.25 are
    exact in double at these B: variance exactly 0), feature 4 has a mean 10^3 times its deviation."""
    g = torch.Generator().manual_seed(seed)
    off = torch.linspace(-1.0, 2.0, H) if H > 1 else torch.tensor([0.4])
    sc = torch.linspace(0.5, 2.0, H) if H > 1 else torch.tensor([1.3])
    y = torch.randn(B, H, generator=g) * sc + off
    gamma, beta = torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g) * 0.5
    if H >= MLP_PLANTS:
        gamma[1], beta[1] = 0.0, 0.0
        gamma[2], beta[2] = 0.0, 0.75
        y[:, 3] = 1.5
        y[:, 4] = torch.randn(B, generator=g) * 0.25 + 250.0
    d = dict(y=y.contiguous(), gamma=gamma, beta=beta, W2=torch.randn(L, H, generator=g) * H ** -0.5, b2=torch.randn(L, generator=g),
             dz=torch.randn(B, L, generator=g) + 0.2, rmean=torch.randn(H, generator=g), rvar=torch.rand(H, generator=g) + 0.5)
    for k, v in d.items():
        assert not bool(((v != 0) & (v.abs() < F32_TINY)).any()), f"subnormal in {k}"
    return d


# ---- the PowerSpherical head in float64 (csrc/vae_head.hip, narrow and wide) --------------------------------------------------------------

class _GivenDirichlet(torch.autograd.Function):
    """torch.distributions.dirichlet._Dirichlet with the draw handed in: forward returns x, backward is _Dirichlet_backward."""

    @staticmethod
    def forward(ctx, conc, x):
        ctx.save_for_backward(x, conc)
        return x.clone()

    @staticmethod
    def backward(ctx, go):
        x, conc = ctx.saved_tensors
        total = conc.sum(-1, True).expand_as(conc)
        grad = torch._dirichlet_grad(x, conc, total)
        return grad * (go - (x * go).sum(-1, True)), None


def _uniform_entropy_f64(L):
    """HypersphericalUniform(L - 1).entropy() as a Python float: the class rounds it to float32 (torch.tensor of a float), 3e-5 at
    L = 512 -- more than the KL's tolerance"""
    return math.log(2) + (L / 2) * math.log(math.pi) - math.lgamma(L / 2)


def _ps_restatement_f64(H2, x, eps, w, w_kl, w_exp):
    """coskad_amd/models/sts/vae.py's head (_finish_heads, PowerSpherical.rsample / entropy, kl_ps_uniform) in float64 on the CPU, on
    the given draws -> (z, kl, 1 / kappa, gradient w.r.t. H2)"""
    import torch.nn.functional as F
    from coskad_amd.models.sts.vae import PowerSpherical
    L = H2.shape[1] - 1
    Hr = H2.double().cpu().clone().requires_grad_(True)
    x, eps, w = x.double().cpu(), eps.double().cpu(), w.double().cpu()
    Z_mean = Hr[:, :L] / torch.norm(Hr[:, :L], dim=-1, keepdim=True)
    Z_var = F.softplus(Hr[:, L:]) + 1
    q = PowerSpherical(loc=Z_mean, scale=Z_var.squeeze(-1))
    zb = _GivenDirichlet.apply(torch.stack([q.alpha, q.beta], -1), x)[..., 0]
    t = (2 * zb - 1).unsqueeze(-1)
    v = F.normalize(eps, dim=-1)
    y = torch.cat([t, torch.sqrt(torch.clamp(1 - t * t, min=0)) * v], -1)
    e1 = torch.zeros_like(Z_mean)
    e1[..., 0] = 1
    u = F.normalize(e1 - Z_mean, dim=-1)
    z = y - 2 * (y * u).sum(-1, keepdim=True) * u
    kl = -q.entropy() + _uniform_entropy_f64(L)
    ik = (1 / Z_var).squeeze(-1)
    ((z * w).sum() + w_kl * kl.sum() + w_exp * ik.sum()).backward()
    return z.detach().numpy(), kl.detach().numpy(), ik.detach().numpy(), Hr.grad.numpy()
