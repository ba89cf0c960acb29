"""csrc/grad_clip.hip through the C ABI: the squared norm of the gradient Adam applies, the two clipping Adam entry points and
the accumulation pass, against float64 numpy.

Sizes: one thread, a ragged block, an exact block, one element past it, more than 256 workgroups (the grid-stride path of the
norm kernel) and the default model's flat buffer."""
import ctypes

import numpy as np
import pytest
import torch

from coskad_amd import _lib, ops

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 65537, 239716]
f32 = lambda x: float(np.float32(x))             # the value the library receives for a float argument
GSCALE, REG = f32(0.5), f32(3e-3)
LR, B1, B2, EPS = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
# beta^t as the steps multiply it up in fp32: the value in front of step 5, and at it
B1P4, B2P4 = f32(np.float32(0.9) ** 4), f32(np.float32(0.999) ** 4)
B1P, B2P = f32(np.float32(B1P4) * np.float32(0.9)), f32(np.float32(B2P4) * np.float32(0.999))
ERR_ARG = -1


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_cache = {}


def inputs(n, masked=True):
    """random g, p, a 0/1 mask and non-zero moments (from a zero state Adam's update is lr * sign(g) whatever the scale of g: a test
    from there would pass without any clipping); computed once per size, never written"""
    if n not in _cache:
        rng = np.random.default_rng(1000 + n)
        _cache[n] = dict(g=rng.standard_normal(n).astype(np.float32), p=rng.standard_normal(n).astype(np.float32),
                         mask=(rng.random(n) < 0.7).astype(np.float32), m=(0.1 * rng.standard_normal(n)).astype(np.float32),
                         v=(0.01 * rng.random(n) + 1e-4).astype(np.float32))
    d = dict(_cache[n])
    if not masked:
        d["mask"] = None
    return d


def g_eff64(d):
    mask = 1.0 if d["mask"] is None else d["mask"].astype(np.float64)
    return d["g"].astype(np.float64) * GSCALE + REG * mask * d["p"].astype(np.float64)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def sqnorm(d):
    part = torch.full((ops.CLIP_PARTIALS,), 7.0, device="cuda", dtype=torch.float64)     # (unused entries must be written 0)
    n = d["g"].size
    rc = _lib.lib().coskad_grad_sqnorm_f32(dev(d["g"]), dev(d["p"]), dev(d["mask"]), n, GSCALE, REG, part, stream())
    assert rc == 0
    return part


def adam64(d, ge):
    """torch.optim.Adam's update in float64 at step 5 on the gradient ge"""
    p, m, v = (d[k].astype(np.float64) for k in ("p", "m", "v"))
    m1 = B1 * m + (1 - B1) * ge
    v1 = B2 * v + (1 - B2) * ge * ge
    return p - LR / (1 - B1P) * (m1 / (np.sqrt(v1) / np.sqrt(1 - B2P) + EPS)), m1, v1


def run_adam(d, entry, clip=None, mode=1, part=None, g=None):
    """entry: 'plain' (coskad_adam_pow_f32), 'pow' / 'dev' (the clipping entry points) -> (p, m, v, norm_out) as numpy"""
    L = _lib.lib()
    p, m, v, mask = dev(d["p"]), dev(d["m"]), dev(d["v"]), dev(d["mask"])
    g = dev(d["g"] if g is None else g)
    n = p.numel()
    norm = torch.full((1,), -1.0, device="cuda")
    if entry == 'plain':
        rc = L.coskad_adam_pow_f32(p, g, m, v, mask, n, LR, B1, B2, EPS, B1P, B2P, GSCALE, REG, stream())
    elif entry == 'pow':
        rc = L.coskad_adam_clip_pow_f32(p, g, m, v, mask, n, LR, B1, B2, EPS, B1P, B2P, GSCALE, REG, part, clip, mode, norm, stream())
    else:
        hyper = torch.tensor([LR, B1P4, B2P4, 0.0], device="cuda", dtype=torch.float32)
        rc = L.coskad_adam_clip_dev_f32(p, g, m, v, mask, n, hyper, B1, B2, EPS, GSCALE, REG, part, clip, mode, norm, stream())
        assert float(hyper[1]) == B1P and float(hyper[2]) == B2P
    assert rc == 0, L.coskad_last_error()
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), float(norm)


def close(got, want, what):
    # the update is ~ lr * O(1) ~ 1e-3 and the fp32 rounding of its few operations stays below 1e-6 of that; m, v and p themselves
    # are rounded to fp32 once (6e-8 relative)
    for a, b, name in zip(got, want, "pmv"):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_sqnorm_vs_float64(n, masked):
    """g_eff is rounded to fp32 (<= 6e-8 relative per element, with or without FMA contraction) and the sum itself is fp64: 1e-6"""
    d = inputs(n, masked)
    part = sqnorm(d)
    want = float((g_eff64(d) ** 2).sum())
    got = part.cpu().numpy()
    print(f"n={n} masked={masked}: sum {got.sum():.17g} float64 {want:.17g} rel {abs(got.sum() - want) / want:.3g}")
    np.testing.assert_allclose(got.sum(), want, rtol=1e-6)
    blocks = min((n + 255) // 256, ops.CLIP_PARTIALS)
    assert (got[blocks:] == 0).all() and (got[:blocks] > 0).all()
    assert torch.equal(part, sqnorm(d))                                 # fixed summation order


@pytest.mark.parametrize("n", SIZES)
def test_plain_adam_meets_the_bound(n):
    """the bound of the clipping tests is one coskad_adam_pow_f32 itself meets against the same float64 Adam"""
    d = inputs(n)
    close(run_adam(d, 'plain')[:3], adam64(d, g_eff64(d)), "adam_pow")


@pytest.mark.parametrize("entry", ['pow', 'dev'])
@pytest.mark.parametrize("n", SIZES)
def test_norm_clip_vs_float64(n, entry):
    d = inputs(n)
    ge = g_eff64(d)
    norm = float(np.sqrt((ge ** 2).sum()))
    part = sqnorm(d)
    for clip in (2.0 * norm, 0.01 * norm):                                # one above the norm, one that bites
        coef = min(1.0, f32(clip) / (norm + 1e-6))
        *pmv, norm_out = run_adam(d, entry, f32(clip), 1, part)
        close(pmv, adam64(d, ge * coef), f"{entry} clip {clip:.4g}")
        if coef < 1 and n > 1:                                            # the test discriminates: the unclipped update is far away
            assert np.abs(adam64(d, ge)[1] - pmv[1]).max() > 1e-4
        want = np.float32(np.sqrt(part.cpu().numpy().sum()))
        assert abs(np.float32(norm_out) - want) <= np.spacing(want)


@pytest.mark.parametrize("entry", ['pow', 'dev'])
@pytest.mark.parametrize("n", SIZES)
def test_value_clip_vs_float64(n, entry):
    d = inputs(n)
    ge = g_eff64(d)
    clip = f32(np.median(np.abs(ge)))
    *pmv, norm_out = run_adam(d, entry, clip, 2, None)                    # no norm launch, partials NULL
    close(pmv, adam64(d, np.clip(ge, -clip, clip)), f"{entry} value clip")
    assert norm_out == -1.0                                               # not written in value mode
    if n > 1:
        assert np.abs(adam64(d, ge)[1] - pmv[1]).max() > 1e-4


@pytest.mark.parametrize("entry", ['pow', 'dev'])
def test_value_clip_keeps_a_nan_gradient(entry):
    """torch.clamp (clip_grad_value_) propagates NaN: a diverged gradient must surface in p, m, v, not turn into -clip_val"""
    d = inputs(257)
    g = d["g"].copy()
    g[[3, 256]] = np.nan
    p, m, v, _ = run_adam(d, entry, f32(0.5), 2, None, g=g)
    bad = np.isnan(g)
    for a in (p, m, v):
        assert np.isnan(a[bad]).all() and np.isfinite(a[~bad]).all()


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_clip_that_never_bites_is_bit_identical(n, masked):
    """clip_val = 1e30: the coefficient is exactly 1 and p, m, v are coskad_adam_pow_f32's bit for bit; the _dev form with the same
    beta^t in device memory agrees with both (the guarantee coskad_adam_pow_f32 documents for the unclipped pair)"""
    d = inputs(n, masked)
    part = sqnorm(d)
    plain = run_adam(d, 'plain')[:3]
    for entry in ('pow', 'dev'):
        got = run_adam(d, entry, f32(1e30), 1, part)[:3]
        for a, b, name in zip(got, plain, "pmv"):
            assert np.array_equal(a, b), f"{entry}: {name} differs from adam_pow"


@pytest.mark.parametrize("n", SIZES)
def test_grad_accum(n):
    L = _lib.lib()
    rng = np.random.default_rng(n)
    g1, g2 = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
    guard = 64
    acc = torch.full((n + guard,), 3.25, device="cuda")
    assert L.coskad_grad_accum_f32(acc, dev(g1), n, 1, stream()) == 0
    assert np.array_equal(acc[:n].cpu().numpy(), g1)                      # first: a copy
    assert L.coskad_grad_accum_f32(acc, dev(g2), n, 0, stream()) == 0
    assert np.array_equal(acc[:n].cpu().numpy(), g1 + g2)                 # then: the fp32 sum, exact against numpy's
    assert bool((acc[n:] == 3.25).all())                                  # nothing beyond n


def test_argument_errors():
    L = _lib.lib()
    n = 300
    t = lambda: torch.zeros(n, device="cuda")
    p, g, m, v, acc = t(), t(), t(), t(), t()
    part = torch.zeros(ops.CLIP_PARTIALS, device="cuda", dtype=torch.float64)
    hyper = torch.tensor([LR, B1P4, B2P4, 0.0], device="cuda")
    s = stream()
    sq = lambda g_, p_, part_, n_: L.coskad_grad_sqnorm_f32(g_, p_, None, n_, 1.0, 0.0, part_, s)
    for bad in ((None, p, part, n), (g, None, part, n), (g, p, None, n), (g, p, part, 0)):
        assert sq(*bad) == ERR_ARG
    assert b"grad_sqnorm" in L.coskad_last_error()
    pw = lambda p_=p, g_=g, m_=m, v_=v, n_=n, part_=part, clip=1.0, mode=1: L.coskad_adam_clip_pow_f32(
        p_, g_, m_, v_, None, n_, LR, B1, B2, EPS, B1P, B2P, 1.0, 0.0, part_, clip, mode, None, s)
    dv = lambda p_=p, g_=g, m_=m, v_=v, n_=n, part_=part, clip=1.0, mode=1, hyper_=hyper: L.coskad_adam_clip_dev_f32(
        p_, g_, m_, v_, None, n_, hyper_, B1, B2, EPS, 1.0, 0.0, part_, clip, mode, None, s)
    for fn in (pw, dv):
        for kw in (dict(p_=None), dict(g_=None), dict(m_=None), dict(v_=None), dict(n_=0), dict(part_=None),
                   dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")), dict(clip=float("inf")), dict(mode=0), dict(mode=3)):
            assert fn(**kw) == ERR_ARG, kw
        assert fn(part_=None, mode=2) == 0                                # value mode needs no partials
    assert dv(hyper_=None) == ERR_ARG
    # nothing was launched by the refused calls: hyper's beta^t moved once, by the one accepted _dev call
    assert float(hyper[1]) == f32(np.float32(B1P4) * np.float32(0.9))
    for bad in ((None, g, n), (acc, None, n), (acc, g, 0)):
        assert L.coskad_grad_accum_f32(*bad, 1, s) == ERR_ARG


@pytest.mark.parametrize("name", ["adam_clip_pow", "adam_clip_dev"])
def test_writing_wrappers_move_the_raw_write_epoch(name, monkeypatch):
    """the wrappers that hand the library parameter pointers to write move ops.raw_write_epoch() (every library call a no-op)"""
    monkeypatch.setattr(ops, "call", lambda *a, **k: None)
    t = lambda: torch.zeros(8, device="cuda")
    part = torch.zeros(ops.CLIP_PARTIALS, device="cuda", dtype=torch.float64)
    before = ops.raw_write_epoch()
    if name == "adam_clip_pow":
        ops.adam_clip_pow(t(), t(), t(), t(), None, LR, B1, B2, EPS, B1P, B2P, part, 1.0)
    else:
        ops.adam_clip_dev(t(), t(), t(), t(), None, torch.zeros(4, device="cuda"), B1, B2, EPS, part, 1.0)
    assert ops.raw_write_epoch() > before
    before = ops.raw_write_epoch()
    ops.grad_sqnorm(t(), t(), None, partials=part)                        # reads the parameters only
    ops.grad_accum(t(), t(), True)                                        # writes no module state
    assert ops.raw_write_epoch() == before
