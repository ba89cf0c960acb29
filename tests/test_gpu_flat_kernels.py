"""Kernel-level checks of the small kernels every flat train step runs: coskad_rec_head_f32 (csrc/stsgcn_fwd.hip),
coskad_adam_pow_f32 / coskad_adam_dev_f32 (csrc/heads.hip) and coskad_gather_transform_f32 (csrc/data.hip), against the float64
restatements of kernel_refs.py (gradients from autograd) or, where the kernel is written to a fixed float32 order, bit for bit against
numpy float32.  Bounds: k * U32 * M as in test_gpu_wide_kernels.py; derivations in the docstrings."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_refs import U32, U64, dd
from test_gpu_wide_kernels import _close

pytestmark = pytest.mark.gpu


# ---- rec_head --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 255, 257, 2 * 12 * 17 * 5, 1024 * 256 + 77])
def test_rec_head(n):
    """loss = mean (PReLU(U) - x)^2, dU, the reconstruction and the slope gradient, for need_grad x need_xrec x upstream in {1, 0.37} x
    dslope fresh / accumulated.  n = 1024 * 256 + 77 is beyond the 1024-block grid: 77 threads take a second element (e = 2).

    r = a v (1 rounding), d = r - x (1): err(d) <= U32 (|r| + |d|).  Sum of squares: fma(d, d, sq) once per element of the thread (e),
    wave_sum (6), the four-wave sum (2), then a double sum and one rounding of the loss: the squares carry 2 |d| err(d) and the sum
    (e + 9) roundings: bound = (2 sum |d| (|r| + |d|) + (e + 9) sum d^2) U32 / n.
    dU = a . (gscale d), gscale = (float)(2 upstream / n): err(d), gscale (1), the product (1), a g (1):
    bound = U32 gscale gate (|r| + 4 |d|), gate = a where v <= 0, 1 elsewhere.
    dslope = sum g v [v < 0]: err(g) |v| with err(g) = U32 gscale (|r| + 3 |d|), the same (e + 9) roundings of the sum on
    sum |g v|, and, accumulating, one more on |prior| + |sum|.
    The reconstruction is compared bit for bit with float32 where(v > 0, v, a v)."""
    from coskad_amd import ops
    g = torch.Generator().manual_seed(n)
    U = torch.randn(n, generator=g)
    x = torch.randn(n, generator=g) * 0.5
    if n >= 3:
        U[0], U[n // 2] = 0.0, -0.0                 # exact zeros: the slope's side of the derivative, no slope gradient
    a32 = np.float32(0.15)
    a = float(a32)
    slope = torch.tensor([a32])
    e = 2 if n > 1024 * 256 else 1
    Ud, xd, sd = U.cuda(), x.cuda(), slope.cuda()
    want_rec = np.where(U.numpy() > 0, U.numpy(), a32 * U.numpy())
    assert want_rec.dtype == np.float32
    for upstream in (1.0, 0.37):
        up = R.f32(upstream)
        U64_ = dd(U).requires_grad_(True)
        a64 = torch.tensor(a, dtype=torch.float64, requires_grad=True)
        loss_ref = R.rec_head(U64_, dd(x), a64)
        dU_ref, da_ref = torch.autograd.grad(loss_ref * up, [U64_, a64])
        v = U64_.detach()
        r = R.prelu(v, a)
        d = r - dd(x)
        gs = 2.0 * up / n
        gate = torch.where(v > 0, torch.ones_like(v), torch.full_like(v, a))
        b_loss = (2 * (d.abs() * (r.abs() + d.abs())).sum() + (e + 9) * (d * d).sum()) * U32 / n + (n + 8) * U64 * float(loss_ref)
        b_dU = U32 * gs * gate * (r.abs() + 4 * d.abs())
        neg = v < 0
        gv = (gs * d.abs() * v.abs())[neg].sum()
        b_da = (U32 * gs * (r.abs() + 3 * d.abs()) * v.abs())[neg].sum() + (e + 9) * U32 * gv + (n + 8) * U64 * gv
        for need_grad in (True, False):
            for need_xrec in (True, False):
                for prior in (None, 0.75):
                    tag = f"rec n{n} up{upstream} g{int(need_grad)} x{int(need_xrec)} acc{int(prior is not None)}"
                    dslope = torch.full((1,), float("nan") if prior is None else prior).cuda()
                    loss, dU, xrec = ops.rec_head(Ud, xd, sd, need_grad=need_grad, need_xrec=need_xrec, dslope=dslope, upstream=upstream,
                                                  accumulate=prior is not None)
                    _close(tag + " loss", loss.cpu().numpy(), loss_ref.detach().reshape(1).numpy(), np.full(1, float(b_loss)))
                    assert (xrec is not None) == need_xrec and (dU is not None) == need_grad
                    if need_xrec:
                        assert np.array_equal(xrec.cpu().numpy(), want_rec)
                    if need_grad:
                        _close(tag + " dU", dU.cpu().numpy(), dU_ref.numpy(), b_dU.numpy())
                        want = float(da_ref) + (prior or 0.0)
                        extra = U32 * (abs(prior) + abs(float(da_ref))) if prior is not None else 0.0
                        _close(tag + " dslope", dslope.cpu().numpy(), np.full(1, want), np.full(1, float(b_da) + extra))
                    else:                                                 # no gradient asked for: the slope gradient is not touched
                        got = dslope.cpu()
                        assert torch.isnan(got).all() if prior is None else float(got) == prior


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------------

LR, B1, B2, AEPS = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)        # as the `float` parameters hold them
GSCALE, REG = R.f32(0.5), R.f32(1e-3)


def _adam_bound(p, g, m, v, mask, t, p_ref, m_ref, v_ref):
    """one step from the float32 state (p, m, v), all double arrays -> bounds of (p, m, v).

    g' = fma(reg mask, p, g gscale): the products round once, the fma once: err(g') <= 2 U32 G, G = |g gscale| + |reg mask p|.
    m' = beta1 m + (1 - beta1) g' (1 - beta is exact in float32 for beta in [0.5, 1]): two products and the add:
    err(m') <= U32 (2 beta1 |m| + 4 (1 - beta1) G).  v' = beta2 v + (1 - beta2) g' g': three roundings on the second term, the add,
    and g' squared carries its error twice: err(v') <= U32 (2 beta2 |v| + 7 (1 - beta2) G^2), rho_v = err(v') / v'.
    The running products beta^t carry t roundings, so bc = 1 - beta^t is off by (t U32 beta^t + U32) / (1 - beta^t) relatively
    (rho_1, rho_2).  denom = sqrt(v') / sqrt(bc2) + eps: rho_v / 2 + sqrt (2) + rho_2 / 2 + sqrt (2) + division (2) + add (1).
    step = lr / bc1: rho_1 + division (2).  upd = step (m' / denom): err(m') step / denom + |upd| (rho_denom + rho_step + 3 U32).
    p' = p - upd: U32 (|p| + |upd|) + err(upd)."""
    G = np.abs(g * GSCALE) + np.abs(REG * (mask if mask is not None else 1.0) * p)
    bm = U32 * (2 * B1 * np.abs(m) + 4 * (1 - B1) * G)
    bv = U32 * (2 * B2 * np.abs(v) + 7 * (1 - B2) * G * G)
    rho_v = bv / np.maximum(v_ref, 1e-300)
    rho1 = (t * B1 ** t + 1) * U32 / (1 - B1 ** t)
    rho2 = (t * B2 ** t + 1) * U32 / (1 - B2 ** t)
    bc1, bc2 = 1 - B1 ** t, 1 - B2 ** t
    denom = np.sqrt(v_ref) / np.sqrt(bc2) + AEPS
    upd = np.abs(LR / bc1 * m_ref / denom)
    rho_denom = rho_v / 2 + rho2 / 2 + 7 * U32
    rho_step = rho1 + 2 * U32
    b_upd = bm * (LR / bc1) / denom + upd * (rho_denom + rho_step + 3 * U32)
    return U32 * (np.abs(p) + upd) + b_upd, bm, bv


@pytest.mark.parametrize("n", [1, 255, 1000])
@pytest.mark.parametrize("masked", [False, True])
def test_adam_pow_and_dev(n, masked):
    """six steps of coskad_adam_pow_f32 (the host multiplies beta^t up in numpy float32) and of coskad_adam_dev_f32 (the device does,
    in `hyper`) from the same start, with reg_coef and gscale set: bitwise equal after every step (the claim in csrc/heads.hip), and
    each step within _adam_bound of kernel_refs.adam_step in double applied to the float32 state the step started from -- with the
    betas, the learning rate and epsilon as the kernels receive them, float(np.float32(0.999)) and not 0.999.  `hyper` must hold
    {lr, beta1^t, beta2^t} as float32 running products after every call."""
    from coskad_amd import ops
    gen = torch.Generator().manual_seed(n + int(masked))
    p0 = torch.randn(n, generator=gen)
    mask = (torch.rand(n, generator=gen) < 0.6).float() if masked else None
    state = {}
    for kind in ("pow", "dev"):
        state[kind] = dict(p=p0.clone().cuda(), m=torch.zeros(n).cuda(), v=torch.zeros(n).cuda())
    hyper = torch.tensor([1e-3, 1.0, 1.0, 0.0]).cuda()
    mk = mask.cuda() if masked else None
    b1pow = b2pow = np.float32(1.0)
    for t in range(1, 7):
        g = torch.randn(n, generator=gen) * (0.1 if t == 3 else 1.0)
        before = {k: dd(x).numpy() for k, x in state["pow"].items()}
        b1pow, b2pow = np.float32(b1pow * np.float32(0.9)), np.float32(b2pow * np.float32(0.999))
        s = state["pow"]
        ops.adam_pow(s["p"], g.cuda(), s["m"], s["v"], mk, 1e-3, 0.9, 0.999, 1e-8, float(b1pow), float(b2pow), gscale=0.5, reg_coef=1e-3)
        s = state["dev"]
        ops.adam_dev(s["p"], g.cuda(), s["m"], s["v"], mk, hyper, 0.9, 0.999, 1e-8, gscale=0.5, reg_coef=1e-3)
        h = hyper.cpu().numpy()
        assert h[0] == np.float32(1e-3) and h[1] == b1pow and h[2] == b2pow and h[3] == 0.0, (t, h)
        for k in ("p", "m", "v"):
            assert torch.equal(state["pow"][k].view(torch.int32), state["dev"][k].view(torch.int32)), (k, t)
        m64 = dd(mask).numpy() if masked else None
        ref = R.adam_step(before["p"], dd(g).numpy(), before["m"], before["v"], t, LR, B1, B2, AEPS, m64, GSCALE, REG)
        bounds = _adam_bound(before["p"], dd(g).numpy(), before["m"], before["v"], m64, t, *ref)
        for k, want, b in zip(("p", "m", "v"), ref, bounds):
            _close(f"adam n{n} mask{int(masked)} step{t} {k}", state["dev"][k].cpu().numpy(), want, b)


def test_adam_dev_two_calls_advance_hyper_twice():
    """replay-style: the step count lives in `hyper`, so two identical calls (same arguments, as a replayed graph makes them) apply
    steps 1 and 2 -- equal to adam_pow at beta and beta^2"""
    from coskad_amd import ops
    gen = torch.Generator().manual_seed(4)
    n = 300
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen).cuda()
    a = dict(p=p0.clone().cuda(), m=torch.zeros(n).cuda(), v=torch.zeros(n).cuda())
    b = dict(p=p0.clone().cuda(), m=torch.zeros(n).cuda(), v=torch.zeros(n).cuda())
    hyper = torch.tensor([1e-3, 1.0, 1.0, 0.0]).cuda()
    b1, b2 = np.float32(0.9), np.float32(0.999)
    for t in (1, 2):
        ops.adam_dev(a["p"], g, a["m"], a["v"], None, hyper, 0.9, 0.999, 1e-8)
        ops.adam_pow(b["p"], g, b["m"], b["v"], None, 1e-3, 0.9, 0.999, 1e-8, float(b1 if t == 1 else np.float32(b1 * b1)),
                     float(b2 if t == 1 else np.float32(b2 * b2)))
    h = hyper.cpu().numpy()
    assert h[1] == np.float32(b1 * b1) and h[2] == np.float32(b2 * b2)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ---- gather_transform ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("TV", [204, 300, 51, 4, 1])
@pytest.mark.parametrize("B", [1, 37, 300])
def test_gather_transform(TV, B):
    """both widths (TV % 4 == 0: four positions per thread; 51 and 1: the scalar kernel), random matrices, N = 11 windows, 5 transforms.
    The indices hold the first and the last valid value, a negative one and one with index // N >= ntrans; the last two give an
    all-zero clip, and every valid clip equals numpy float32 (x m0 + y m1) + m2 bit for bit (the kernel is written to that order and
    built without FMA contraction).  B = 1 runs each of the four special indices on its own."""
    from coskad_amd import ops
    N, ntrans = 11, 5
    gen = torch.Generator().manual_seed(TV * 1000 + B)
    xy = torch.randn(N, 2, TV, generator=gen)
    mats = torch.randn(ntrans, 3, 3, generator=gen)
    special = [0, N * ntrans - 1, -1, N * ntrans, -N * ntrans - 3, N * ntrans + 7]
    if B == 1:
        batches = [[i] for i in special]
    else:
        idx = torch.randint(0, N * ntrans, (B,), generator=gen).tolist()
        for k, i in enumerate(special):
            idx[k * 7 + 1 if k else 0] = i
        batches = [idx]
    for idx in batches:
        index = torch.tensor(idx, dtype=torch.int64)
        out = ops.gather_transform(xy.cuda(), mats.cuda(), index.cuda(), 1, TV).cpu().numpy().reshape(len(idx), 2, TV)
        want = R.gather_transform_f32(xy.numpy(), mats.numpy(), idx, N, ntrans)
        assert out.dtype == want.dtype == np.float32
        assert np.array_equal(out, want), np.argwhere(out != want)[:4]
        for b, i in enumerate(idx):
            if i < 0 or i // N >= ntrans:
                assert not out[b].any()
            else:
                assert out[b].any()
