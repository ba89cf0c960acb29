"""Kernel-level checks of the one-class heads and their centres: csrc/heads.hip (L <= 16, one thread per clip; 16 < L <= 512, one wave
per clip) and the MFMA Mahalanobis head and Gram of csrc/heads_wide.hip, called directly with guard bands around every output.  The value compared with is always
oracle/ref_cpu.py evaluated in double on the float32 inputs, gradients from autograd on that forward.  Bounds: for the Euclidean and
Mahalanobis heads, the Gram matrix, sqnorm and the finalizers k * U32 * M derived by hand in the docstrings (plus (count + 8) * U64 * M
where the kernel sums in double); for the Poincare chain the running-error arithmetic of kernel_refs.py, which restates the kernels'
operation sequence once and is held to the oracle and to numpy float32 by test_kernel_refs_host.py.  Nothing is fitted to the
kernels' output.  Inputs: kernel_refs.head_inputs (radii on both sides of every clamp, centres up to |c| = 0.995)."""
import numpy as np
import pytest
import torch

import kernel_refs as K
from kernel_refs import U32, U64, dd
from oracle import ref_cpu as O
from test_gpu_wide_kernels import _close
from test_gpu_wide_latent import SENT, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

NARROW = [(L, B) for L in (1, 2, 5, 15, 16) for B in (1, 63, 65, 511, 512, 513, 1029)]
WIDE = ([(L, B) for L in (17, 33, 64, 65, 256, 257, 512) for B in (1, 5, 17, 67)]
        + [(L, B) for L in (17, 65) for B in (15, 16, 16384, 16384 + 19)])       # the last B: a second grid-stride round
SHAPES = NARROW + WIDE
SIZES = dict(dz=lambda B, L, S: B * L, zh=lambda B, L, S: B * L, score=lambda B, L, S: B, stats=lambda B, L, S: S)


def _head(kind, z, c, VI=None, acc=None, gram=None, gram_accumulate=1, upstream=1.0, absent=()):
    """one C-ABI call with guarded outputs (those in `absent` passed as NULL) -> dict of host tensors"""
    from coskad_amd import ops
    from coskad_amd._lib import call
    B, L = z.shape
    S = ops.head_slots(L)
    names = ("dz", "zh", "score", "stats") if kind == "poincare" else ("dz", "score", "stats")
    bufs = {k: _guarded(SIZES[k](B, L, S)) for k in names if k not in absent}
    o = lambda k: bufs[k][1] if k in bufs else None
    ws = ops.head_ws(B, z.device, L)
    st = ops._stream()
    if kind == "mse":
        call("coskad_mse_head_f32", z, c, o("dz"), o("score"), o("stats"), acc, upstream, ws, B, L, st)
    elif kind == "maha":
        call("coskad_mahalanobis_head_f32", z, c, VI, o("dz"), o("score"), o("stats"), acc, gram, int(gram_accumulate), upstream, ws,
             B, L, st)
    else:
        call("coskad_poincare_head_f32", z, c, o("dz"), o("zh"), o("score"), o("stats"), acc, upstream, ws, B, L, st)
    torch.cuda.synchronize()
    for k, (b, _) in bufs.items():
        _guards_intact(b, f"{kind} {k}")
    return {k: bufs[k][1].cpu().clone() for k in bufs}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, keys, tag):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{tag}: {k} differs"


def _acc(S, prior=0.25):
    return torch.full((S,), prior, device="cuda")


def _sum_bound(terms_abs_sum, err_sum, ks, P):
    """a slot's raw sum over the clips: the terms' own errors, ks float32 roundings on the sum of their magnitudes, the double sum of
    the P partial rows"""
    return err_sum + ks * U32 * terms_abs_sum + (P + 8) * U64 * terms_abs_sum


def _acc_two_calls(tag, acc, raw_ref, b_raw, prior=0.25):
    """acc after two calls onto `prior`: fl(fl(prior + s) + s) with s the call's raw sum (within b_raw of raw_ref)"""
    want = prior + 2 * raw_ref
    bound = 2 * b_raw + U32 * ((prior + raw_ref).abs() + want.abs())
    _close(tag, acc.cpu().numpy(), want.numpy(), bound.numpy())


def _modes(kind, z, c, full, S, tag, **kw):
    """calling modes shared by the three heads: every output absent in turn (the others bit-equal to the full call), a repeat call
    bitwise equal including stats and acc"""
    outs = [k for k in full]
    for drop in outs + ["acc"]:
        acc = None if drop == "acc" else _acc(S)
        got = _head(kind, z, c, acc=acc, absent=(drop,), **kw)
        assert drop == "acc" or drop not in got
        _same(got, full, [k for k in outs if k != drop], f"{tag} without {drop}")
    a1, a2 = _acc(S), _acc(S)
    r1, r2 = _head(kind, z, c, acc=a1, **kw), _head(kind, z, c, acc=a2, **kw)
    _same(r1, r2, outs, tag + " repeat")
    _same(r1, full, outs, tag + " repeat vs first")
    assert torch.equal(_bits(a1), _bits(a2)), tag + " repeat: acc differs"


def test_head_workspace_steps_at_the_single_block_boundary():
    """one partial row up to 512 clips, two from 513 (coskad_head_ws_floats): the B = 511 / 512 / 513 cases below straddle the boundary
    the library reports, between the block that writes stats / acc itself and the partial rows + k_head_finalize"""
    from coskad_amd import _lib, ops
    lib = _lib.lib()
    S = ops.head_slots(16)
    assert lib.coskad_head_ws_floats(512) == S and lib.coskad_head_ws_floats(513) == 2 * S
    assert K.head_blocks(512, 16) == 1 and K.head_blocks(513, 16) == 2 and K.HEAD_ROWS == 512
    assert lib.coskad_head_ws_floats_l(16384, 17) == lib.coskad_head_ws_floats_l(16384 + 19, 17) == 1024 * ops.head_slots(17)


# ---- Poincare head -----------------------------------------------------------------------------------------------------------------------

def _poincare_ref(z, c, upstream):
    zd = z.double().requires_grad_(True)
    loss, zh = O.poincare_loss(zd, c.double())
    (gz,) = torch.autograd.grad(loss * K.f32(upstream), zd)
    zh = zh.detach()
    return loss.detach(), zh, O.dist(c.double()[None], zh), gz


def _assert_margins(A, tag):
    """the cap on rows left out is 0: every row lies further from every select's threshold than the two sides' bounds"""
    for name, margin, bound in A.margins:
        assert bool((margin > bound).all()), (tag, name, float((margin - bound).min()))


@pytest.mark.parametrize("L,B", SHAPES)
def test_poincare_head(L, B):
    """k_poincare_head<PerThread> / <PerWave> at the four centres |c| in {0, 0.4, 0.93, 0.995} and without a centre.

    zh, score and dz per element against the oracle within the running-error bound of kernel_refs.poincare_head_chain (dz for
    upstream in {1, 0.37, B}; the other outputs do not depend on upstream: bit-equal).  Slot sums: a clip's term t_n carries its chain
    bound; the sum adds ks = kernel_refs.head_sum_roundings(B, L) float32 roundings of sum |t_n| and the double sum of the P partial
    rows.  stats[0] = raw sum * scale0 with scale0 = 1.f / (float)B: two more roundings.  Slots L+1 .. 16 of a narrow head stay 0.
    acc: two calls onto a prior of 0.25, fl(fl(prior + s) + s).  Without a centre: zh bit-equal, the sums bit-equal, stats[0] = 0, dz
    and score untouched."""
    from coskad_amd import ops
    wide = L > K.HEAD_LMAX
    S, Lp, P, ks = ops.head_slots(L), max(L, 16), K.head_blocks(B, L), K.head_sum_roundings(B, L)
    for ci, cnorm in enumerate(K.HEAD_CENTRES):
        tag = f"poincare L{L} B{B} c{cnorm}"
        z, c = K.head_inputs(B, L, cnorm, seed=ci)
        zc, cc = z.cuda(), c.cuda()
        loss, zh, d, g1 = _poincare_ref(z, c, 1.0)
        assert torch.isfinite(g1).all()
        # one chain per centre: from gscale on every operation is linear in it and every rounding relative, so the bound of dz at
        # gscale = upstream / (float)B is f32(upstream) times the bound at 1 / B taken with the division's one rounding
        A = K.EVMath()
        ev = K.poincare_head_chain(A, z, c, wide, (1.0 / B, (1.0 + U32) / B))
        _assert_margins(A, tag)
        full = None
        for upstream in (1.0, 0.37, float(B)):
            acc = _acc(S)
            out = _head("poincare", zc, cc, acc=acc, upstream=upstream)
            gz, b_dz = g1 * K.f32(upstream), ev["dz"].e * K.f32(upstream)
            _close(f"{tag} up{upstream} dz", out["dz"].view(B, L).numpy(), gz.numpy(), b_dz.numpy())
            if full is not None:
                _same(out, full, ("zh", "score", "stats"), tag + f" upstream {upstream}")
                continue
            full = out
            _close(tag + " zh", out["zh"].view(B, L).numpy(), zh.numpy(), ev["zh"].e.numpy())
            _close(tag + " score", out["score"].numpy(), d.numpy(), ev["d"].e[:, 0].numpy())
            # raw slot sums, their references and bounds
            Sv, sa, sb = K.poincare_slot_sums(zh)
            raw = torch.zeros(S, dtype=torch.float64)
            b_raw = torch.zeros(S, dtype=torch.float64)
            raw[0], b_raw[0] = d.sum(), _sum_bound(d.abs().sum(), ev["d"].e.sum(), ks, P)
            raw[1:1 + L], b_raw[1:1 + L] = Sv, _sum_bound(ev["gzh"].v.abs().sum(0), ev["gzh"].e.sum(0), ks, P)
            raw[Lp + 1], b_raw[Lp + 1] = sa, _sum_bound(ev["gm1"].v.abs().sum(), ev["gm1"].e.sum(), ks, P)
            raw[Lp + 2], b_raw[Lp + 2] = sb, _sum_bound(ev["norm"].v.abs().sum(), ev["norm"].e.sum(), ks, P)
            want, b_stats = raw.clone(), b_raw.clone()
            want[0], b_stats[0] = loss, b_raw[0] / B + 2 * U32 * float(loss)
            _close(tag + " stats", out["stats"].numpy(), want.numpy(), b_stats.numpy())
            assert not out["stats"][1 + L:Lp + 1].any()
            _head("poincare", zc, cc, acc=acc)
            _acc_two_calls(tag + " acc", acc, raw, b_raw)
        _modes("poincare", zc, cc, full, S, tag)
        # centre initialisation: c == NULL
        acc0, accn = _acc(S, 0.0), _acc(S, 0.0)
        _head("poincare", zc, cc, acc=acc0)
        none = _head("poincare", zc, None, acc=accn)
        assert bool((none["dz"] == SENT).all()) and bool((none["score"] == SENT).all()), tag + ": written without a centre"
        assert torch.equal(_bits(none["zh"]), _bits(full["zh"])) and torch.equal(_bits(none["stats"][1:]), _bits(full["stats"][1:]))
        assert float(none["stats"][0]) == 0.0 and float(accn[0]) == 0.0
        assert torch.equal(_bits(accn[1:].cpu()), _bits(acc0[1:].cpu()))


@pytest.mark.parametrize("L", [1, 2, 5, 15, 16, 17, 33, 64, 65, 256, 257, 512])
def test_poincare_dist_and_logmap0(L):
    """coskad_poincare_dist_f32 and coskad_poincare_logmap0_f32 on the head's own zh (67 rows) and on points of norm 0, 1e-6 (below
    logmap0's norm clamp), 0.5 and 0.999, against oracle dist / logmap0 of those float32 points within the running-error bound of
    kernel_refs.poincare_dist / logmap0_chain (the points are inputs here: no error of their own)"""
    from coskad_amd import ops
    wide = L > K.HEAD_LMAX
    for ci, cnorm in enumerate(K.HEAD_CENTRES):
        z, c = K.head_inputs(67, L, cnorm, seed=ci)
        zh = _head("poincare", z.cuda(), c.cuda())["zh"].view(67, L)
        g = torch.Generator().manual_seed(L + ci)
        dirs = torch.randn(16, L, generator=g, dtype=torch.float64)
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        norms = torch.tensor([0.0, 1e-6, 0.5, 0.999], dtype=torch.float64).repeat(4)
        y = torch.cat([zh, (dirs * norms[:, None]).float()])
        A = K.EVMath()
        d, _, _ = K.poincare_dist(A, K._row(A, c), A.inp(y), wide, need_grad=False)
        lm = K.logmap0_chain(A, y, wide)
        tag = f"L{L} c{cnorm}"
        score = ops.poincare_dist(y.cuda(), c.cuda()).cpu()
        _close(tag + " poincare_dist", score.numpy(), O.dist(c.double()[None], y.double()).numpy(), d.e[:, 0].numpy())
        _close(tag + " logmap0", ops.poincare_logmap0(y.cuda()).cpu().numpy(), O.logmap0(y.double()).numpy(), lm.e.numpy())


# ---- Euclidean head ----------------------------------------------------------------------------------------------------------------------

def _maha_ks(B, L):
    """hw::k_mahalanobis_wide sums a block's 16-clip tiles in clip order in one thread (s0, the column sums): 16 per tile, the
    conversion; the narrow kernel sums as the other narrow heads"""
    if L <= K.HEAD_LMAX:
        return K.head_sum_roundings(B, L)
    tiles = -(-B // K.WIDE_TILE)
    return 16 * -(-tiles // K.head_blocks(B, L)) + 1


def _euclid_sums(z, ks, P, L, S):
    """reference and bound of slots 1.. of the Euclidean / Mahalanobis heads: sum z (ks roundings on sum |z_nj|), the exact count,
    sum |z_n| (|z_n| = sqrt(dot): (kd / 2 + 1) U32 |z_n| each, kd = dot_roundings(L))"""
    Lp = max(L, 16)
    zd = z.double()
    Sv, n, nb, _ = K.euclid_slot_sums(zd)
    raw, b = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    raw[1:1 + L], b[1:1 + L] = Sv, _sum_bound(zd.abs().sum(0), 0.0, ks, P)
    raw[Lp + 1] = n
    raw[Lp + 2], b[Lp + 2] = nb, _sum_bound(nb, (K.dot_roundings(L) / 2 + 1) * U32 * nb, ks, P)
    return raw, b


@pytest.mark.parametrize("L,B", SHAPES)
def test_mse_head(L, B):
    """k_mse_head<PerThread> / <PerWave>.  d = u - c rounds once; sq = sum d^2 is an fmaf chain (kd = dot_roundings(L) roundings: L fmaf, or
    the lane's ceil(L / 64) and wave_sum's 6) of terms that carry d's rounding twice: err(sq) <= (kd + 2) U32 sq.
    score = sq / (float)L: (kd + 3) U32 score.
    dz = 2 d gscale, gscale = upstream / ((float)B (float)L): the product B L, the division, d and the product round (2 d is exact):
    4 U32 |dz|.
    stats[0] = (sum sq) scale0: the clips' err(sq), the sum's ks roundings (kernel_refs.head_sum_roundings) and the double sum of the
    partial rows, then scale0 = 1.f / ((float)B (float)L) (2 roundings) and the product (1).  The other slots: _euclid_sums."""
    from coskad_amd import ops
    kd, S, Lp, P, ks = K.dot_roundings(L), ops.head_slots(L), max(L, 16), K.head_blocks(B, L), K.head_sum_roundings(B, L)
    z, c = K.head_inputs(B, L, 0.4, seed=1)
    zc, cc = z.cuda(), c.cuda()
    tag = f"mse L{L} B{B}"
    zd = z.double().requires_grad_(True)
    loss = O.mse_to_center(zd, c.double())
    (g1,) = torch.autograd.grad(loss, zd)
    score = O.euclid_window_score(z.double(), c.double())
    sq = score * L
    full = None
    for upstream in (1.0, 0.37, float(B)):
        acc = _acc(S)
        out = _head("mse", zc, cc, acc=acc, upstream=upstream)
        gz = g1 * K.f32(upstream)
        _close(f"{tag} up{upstream} dz", out["dz"].view(B, L).numpy(), gz.numpy(), (4 * U32 * gz.abs()).numpy())
        if full is not None:
            _same(out, full, ("score", "stats"), tag + f" upstream {upstream}")
            continue
        full = out
        _close(tag + " score", out["score"].numpy(), score.numpy(), ((kd + 3) * U32 * score).numpy())
        raw, b_raw = _euclid_sums(z, ks, P, L, S)
        raw[0], b_raw[0] = sq.sum(), _sum_bound(sq.sum(), (kd + 2) * U32 * sq.sum(), ks, P)
        want, b_stats = raw.clone(), b_raw.clone()
        want[0], b_stats[0] = loss.detach(), b_raw[0] / (B * L) + 3 * U32 * float(loss.detach())
        _close(tag + " stats", out["stats"].numpy(), want.numpy(), b_stats.numpy())
        assert float(out["stats"][Lp + 1]) == B and not out["stats"][1 + L:Lp + 1].any()
        _head("mse", zc, cc, acc=acc)
        _acc_two_calls(tag + " acc", acc, raw, b_raw)
    _modes("mse", zc, cc, full, S, tag)


# ---- Mahalanobis head and the Gram matrix ----------------------------------------------------------------------------------------------

def _vi(L, g):
    """SPD plus a 1 % random part: not symmetric, so (VI + VI^T) matters"""
    A = torch.randn(L, L, generator=g) / L ** 0.5
    return (A @ A.T + 0.5 * torch.eye(L) + 0.01 * torch.randn(L, L, generator=g)).float()


def _gram_check(tag, got, z, prior, accumulate):
    """gram (+)= sum_n z_n z_n^T: one fmaf (or MFMA) chain over the B clips in order per entry: B U32 sum_n |z_ni z_nj|, and
    accumulating one more rounding of prior + sum; not accumulating, the prior is overwritten"""
    zd = z.double()
    G = zd.T @ zd
    M = zd.abs().T @ zd.abs()
    want = G + prior if accumulate else G
    bound = z.shape[0] * U32 * M + (U32 * want.abs() if accumulate else 0.0)
    _close(tag, got.cpu().numpy(), want.numpy(), bound.numpy())


@pytest.mark.parametrize("L,B", SHAPES)
def test_mahalanobis_head(L, B):
    """k_mahalanobis_head / hw::k_mahalanobis_wide with a non-symmetric VI; row 2 is the centre itself (B >= 3).

    d = u - c rounds once.  w_r = sum_q VI_rq d_q is a chain of L fmaf (narrow) or of ceil(L / 4) MFMA steps of four chained
    products (wide): err(w_r) <= (L + 1) U32 W_r, W_r = sum_q |VI_rq| |d_q|; likewise wt_j with Wt_j = sum_r |VI_rj| |d_r|.
    q = d . w: d's rounding, w's error and the dot's own chain (k2 = L narrow; wide at most 8 fmaf over the wave's tiles, 4 shuffle
    adds, 3 wave adds = 15): err(q) <= (L + 2 + k2) U32 Q, Q = sum_r |d_r| W_r.
    dist = sqrt(q): e_dist = err(q) / (dist + sqrt(q - err(q))) + U32 dist.
    dz_j = (w_j + wt_j) inv, inv = gscale / (2 dist), gscale = upstream / (float)B: e_s = (L + 1) U32 (W_j + Wt_j) + U32 |s_j|;
    inv: e_dist / (dist - e_dist) + 2 U32 (gscale, the division); the product: bound = |inv| e_s + |s_j inv| (rel(dist) + 3 U32).
    stats[0] = (sum dist) / B: the clips' e_dist, ks roundings (_maha_ks), scale0 and the product (2).
    The row at the centre: d = 0 exactly, so score 0, and dz = (0 + 0) * (gscale / 0) = NaN in the whole row, as torch.sqrt's backward
    gives; it adds 0 to stats[0] and leaves every other row alone."""
    from coskad_amd import ops
    S, Lp, P, ks = ops.head_slots(L), max(L, 16), K.head_blocks(B, L), _maha_ks(B, L)
    k2 = L if L <= K.HEAD_LMAX else 15
    z, c = K.head_inputs(B, L, 0.4, seed=2)
    if B >= 3:
        z[2] = c
    g = torch.Generator().manual_seed(L)
    VI = _vi(L, g)
    zc, cc, vc = z.cuda(), c.cuda(), VI.cuda()
    tag = f"maha L{L} B{B}"
    zd = z.double().requires_grad_(True)
    dist = O.mahalanobis(zd, c.double()[None], VI.double())
    (g1,) = torch.autograd.grad(dist.mean(), zd)
    dist = dist.detach()
    at_c = torch.zeros(B, dtype=torch.bool)
    if B >= 3:
        at_c[2] = True
        assert float(dist[2]) == 0.0 and torch.isnan(g1[2]).all()
    assert torch.isfinite(g1[~at_c]).all()
    d = (z.double() - c.double()[None]).abs()
    Va = VI.double().abs()
    W, Wt = d @ Va.T, d @ Va
    Q = (d * W).sum(1)
    e_q = (L + 2 + k2) * U32 * Q
    e_dist = e_q / (dist + torch.sqrt((dist * dist - e_q).clamp_min(0.0))).clamp_min(1e-300) + U32 * dist
    e_dist[at_c] = 0.0
    full = None
    for upstream in (1.0, 0.37, float(B)):
        acc = _acc(S)
        gram = torch.full((L, L), 0.5, device="cuda")
        out = _head("maha", zc, cc, VI=vc, acc=acc, gram=gram, gram_accumulate=1, upstream=upstream)
        gs = K.f32(upstream) / B
        gz = g1 * K.f32(upstream)
        dv = z.double() - c.double()[None]
        s = dv @ VI.double().T + dv @ VI.double()
        inv = gs / (2 * dist.clamp_min(1e-300))[:, None]
        b_dz = inv * ((L + 1) * U32 * (W + Wt) + U32 * s.abs()) + (s * inv).abs() * (e_dist / (dist - e_dist).clamp_min(1e-300) + 3 * U32)[:, None]
        got = out["dz"].view(B, L)
        assert torch.isnan(got[at_c]).all(), tag + ": the row at the centre must be NaN"
        _close(f"{tag} up{upstream} dz", got[~at_c].numpy(), gz[~at_c].numpy(), b_dz[~at_c].numpy())
        if full is not None:
            _same(out, full, ("score", "stats"), tag + f" upstream {upstream}")
            continue
        full = out
        _close(tag + " score", out["score"].numpy(), dist.numpy(), e_dist.numpy())
        assert bool((out["score"][at_c] == 0).all())
        _gram_check(tag + " gram accumulated", gram, z, 0.5, True)
        raw, b_raw = _euclid_sums(z, ks, P, L, S)
        raw[0], b_raw[0] = dist.sum(), _sum_bound(dist.sum(), e_dist.sum(), ks, P)
        want, b_stats = raw.clone(), b_raw.clone()
        want[0], b_stats[0] = dist.mean(), b_raw[0] / B + 2 * U32 * float(dist.mean())
        _close(tag + " stats", out["stats"].numpy(), want.numpy(), b_stats.numpy())
        assert float(out["stats"][Lp + 1]) == B and not out["stats"][1 + L:Lp + 1].any()
        _head("maha", zc, cc, VI=vc, acc=acc)
        _acc_two_calls(tag + " acc", acc, raw, b_raw)
        gram0 = torch.full((L, L), 0.5, device="cuda")
        _head("maha", zc, cc, VI=vc, gram=gram0, gram_accumulate=0)
        _gram_check(tag + " gram overwritten", gram0, z, 0.5, False)
    # calling modes: NaN rows compare as bit patterns
    _modes("maha", zc, cc, full, S, tag, VI=vc)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("L", [5, 16, 33])
@pytest.mark.parametrize("B", [255, 257, 513])
def test_gram_around_the_lds_chunk(B, L, accumulate):
    """k_gram stages 256 clips per LDS chunk: B = 255 / 257 / 513 are one short chunk, one full + 1 clip, two full + 1; onto a non-zero
    prior, accumulated and overwritten (L = 33: hw::k_gram_wide, 3 x 3 tiles with ragged edges)"""
    z, c = K.head_inputs(B, L, 0.4, seed=4)
    gram = torch.full((L, L), -0.75, device="cuda")
    VI = _vi(L, torch.Generator().manual_seed(L))
    _head("maha", z.cuda(), c.cuda(), VI=VI.cuda(), gram=gram, gram_accumulate=accumulate)
    _gram_check(f"gram B{B} L{L} acc{accumulate}", gram, z, -0.75, bool(accumulate))


# ---- finalizers ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 12, 16, 17, 512])
def test_center_finalize(L):
    """c = S / n rounds once (U32 |c|), then |c| < eps -> +-eps.  eps = 0.25 is exact in float32 and n = 7 leaves most quotients inexact
    (+-eps themselves come out exact: 1.75 / 7); the entries cycle through values inside eps of both signs (clamped to +-eps exactly),
    +0.0 and -0.0 (pass through, sign kept), exactly +-eps (unchanged) and values well outside; |S / n| is either exactly eps or at
    least 20 % away from it"""
    from coskad_amd import ops
    eps, n = 0.25, 7.0
    vals = torch.tensor([0.1, -0.1, 0.0, -0.0, 0.25, -0.25, 3.0, -7.5, 1e-3, -1e-20, 0.3, -0.2, 0.2000001, 1e-30], dtype=torch.float32)
    cvals = vals[torch.arange(L) % len(vals)]
    S, Lp = ops.head_slots(L), max(L, 16)
    acc = torch.full((S,), 7.0)
    acc[1:1 + L] = cvals * n
    acc[Lp + 1] = n
    got = ops.center_finalize(acc.cuda(), eps, L).cpu()
    want = O.clamp_center(acc[1:1 + L].double() / n, eps)
    _close(f"center_finalize L{L}", got.numpy(), want.numpy(), (U32 * want.abs()).numpy())
    inside = (cvals.abs() < eps) & (cvals != 0)
    assert bool((got[inside].abs() == eps).all()) and bool((torch.sign(got[inside]) == torch.sign(cvals[inside])).all())
    zero = cvals == 0
    assert bool((got[zero] == 0).all()) and torch.equal(torch.signbit(got[zero]), torch.signbit(cvals[zero]))
    edge = cvals.abs() == eps
    assert torch.equal(got[edge], cvals[edge])


@pytest.mark.parametrize("L", [1, 16, 17, 512])
def test_midpoint_finalize(L):
    """the gyromidpoint from synthetic sums, computed in double by the kernel and rounded once: U32 |c| (+ 64 U64 for the order of the
    double operations).  All-zero sums (s clamps to 1e-10, the norm to 1e-15: the centre is exactly 0), s below 1e-10, |S / s| >= 1
    (the 1 - 1e-7 guard: the centre has norm tanh(artanh(1 - 1e-7) / 2)) and ordinary sums; reference:
    kernel_refs.midpoint_from_sums, the oracle's weighted_midpoint from its two sums (held equal on the host)"""
    from coskad_amd import ops
    S, Lp = ops.head_slots(L), max(L, 16)
    g = torch.Generator().manual_seed(L)
    u = torch.randn(L, generator=g, dtype=torch.float64)
    u = u / u.norm()
    z, c = K.head_inputs(67, L, 0.4, seed=5)
    zh = O.poincare_loss(z.double(), c.double())[1]
    Sv, sa, _ = K.poincare_slot_sums(zh)
    cases = dict(zero=(torch.zeros(L, dtype=torch.float64), 0.0), tiny_s=(1e-11 * u, 1e-12), outside=(3.0 * 40.0 * u, 40.0),
                 at_one=(40.0 * u, 40.0), ordinary=(Sv, float(sa)), inside=(0.37 * 25.0 * u, 25.0))
    for name, (vec, s) in cases.items():
        acc = torch.full((S,), 7.0)
        acc[1:1 + L] = vec.float()
        acc[Lp + 1] = s
        got = ops.midpoint_finalize(acc.cuda(), L).cpu()
        want = K.midpoint_from_sums(acc[1:1 + L].double(), acc[Lp + 1].double())
        assert torch.isfinite(want).all()
        _close(f"midpoint_finalize L{L} {name}", got.numpy(), want.numpy(), (U32 * want.abs() + 64 * U64).numpy())
        if name == "zero":
            assert not got.any()
        if name == "outside":
            assert abs(float(got.double().norm()) - float(np.tanh(0.5 * np.arctanh(1 - 1e-7)))) < 1e-6


# ---- sqnorm ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 65536 + 77])
def test_sqnorm(n, masked):
    """out = scale sum mask p^2.  A thread's elements (e = 2 beyond the 256-block grid, n = 65 536 + 77) go through
    fmaf(mask v, v, s) (mask v rounds once when masked), wave_sum (6), (sh0 + sh1) + (sh2 + sh3) (2), the double sum of the blocks'
    partials times scale, one conversion: (e + 9 + masked) U32 M + (blocks + 8) U64 M, M = |scale| sum |mask| p^2"""
    from coskad_amd import ops
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g)
    mask = torch.rand(n, generator=g) if masked else None
    if masked and n > 2:
        mask[0], mask[n // 2] = 0.0, 1.0
    scale = 0.5 / 7
    ws_buf, ws = _guarded(256)
    out = ops.sqnorm(p.cuda(), mask.cuda() if masked else None, scale, ws=ws).cpu()
    _guards_intact(ws_buf, "sqnorm ws")
    terms = (dd(mask) if masked else 1.0) * dd(p) ** 2
    blocks = min(-(-n // 256), 256)
    e = -(-n // (blocks * 256))
    M = abs(K.f32(scale)) * float(terms.abs().sum())
    _close(f"sqnorm n{n} mask{int(masked)}", out.numpy(), np.full(1, K.f32(scale) * float(terms.sum())),
           np.full(1, (e + 9 + int(masked)) * U32 * M + (blocks + 8) * U64 * M))
