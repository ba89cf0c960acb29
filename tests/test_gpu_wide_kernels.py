"""Kernel-level checks of csrc/wide.hip (coskad_bn2_stats_f32, coskad_bn2_apply_prelu_f32, coskad_bn2_bwd_f32,
coskad_dropout_mask_f32) and of coskad_bn2_stats_parts_f32 (csrc/conv1x1.hip) against the float64 restatements of kernel_refs.py,
whose gradients are torch autograd's.  Every bound has the form  k * U32 * M  (U32 = 2^-24, one float32 rounding; M the double sum of the
absolute values of the terms of the element; k the number of roundings on the longest float32 chain, read from the kernel) plus a
(count + 8) * 2^-53 * M term for what the kernels sum in double; the derivations stand in the docstrings.  Each check prints
`RATIO <name> <largest error / bound>` (pytest -rP shows it; DESIGN.md 6.1 records a run)."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_refs import U32, U64, dd

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
EPS_K, MOM_K = R.f32(EPS), R.f32(MOM)         # what the `float eps, float momentum` parameters hold


def _close(name, got, ref, bound, where=None):
    """|got - ref| <= bound elementwise (`where`: the elements compared); prints the largest error / bound ratio"""
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    bound = np.broadcast_to(bound, ref.shape)
    err = np.abs(got - ref)
    if where is not None:
        err, bound = err[where], bound[where]
    ratio = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    print(f"RATIO {name} {ratio:.3f}")
    assert np.all(np.isfinite(got)), name
    assert ratio <= 1.0, (name, ratio)
    return ratio


def _channel_data(Nb, C, P, seed):
    """standard-normal values with a per-channel offset and scale (a zero-mean input would hide every term that multiplies the mean)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(Nb, C, P, generator=g)
    off = torch.linspace(-1.5, 2.5, C) if C > 1 else torch.tensor([0.7])
    sc = torch.linspace(0.5, 2.0, C) if C > 1 else torch.tensor([1.3])
    return (x * sc[None, :, None] + off[None, :, None]).contiguous(), g


def _bn(C, g, track=True):
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM, track_running_stats=track)
    if track:
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(41)
    return bn.cuda()


def _stats_ref(x, rm0, rv0):
    """double statistics of x [N, C, P] and their bounds.

    The kernel sums x and x^2 in double (relative error <= count 2^-53 each), forms mean = s / count and
    var = q / count - mean^2 in double and rounds each result to float32 once: k = 2 (the rounding, and one spare for the product
    with momentum in the running update) on M = |value|, plus the double term: (count + 8) 2^-53 mean|x| for the mean,
    dvar = 2 (count + 8) 2^-53 (mean(x^2) + mean^2) for the variance, the latter carried into invstd through
    |d invstd / d var| = invstd / (2 (var + eps)).  The running values are (1 - momentum) old + momentum new in double, rounded
    once: M = |(1 - momentum) old| + |momentum new|."""
    Nb, C, P = x.shape
    count = Nb * P
    x64 = dd(x)
    mean, var, _ = R.bn_batch_stats(x64, EPS_K)
    inv = 1.0 / torch.sqrt(var + EPS_K)
    absx, sq = x64.abs().mean((0, 2)), (x64 * x64).mean((0, 2))
    dbl = (count + 8) * U64
    dvar = 2 * dbl * (sq + mean * mean)
    ref = {"mean": mean, "inv": inv}
    bound = {"mean": 2 * U32 * mean.abs() + dbl * absx, "inv": 2 * U32 * inv + 0.5 * inv / (var + EPS_K) * dvar}
    if rm0 is not None:
        rm, rv = R.bn_running_update(mean, var, count, dd(rm0), dd(rv0), MOM_K)
        unb = var * count / (count - 1.0) if count > 1 else var
        ref.update(rm=rm, rv=rv)
        bound["rm"] = 2 * U32 * ((1 - MOM_K) * dd(rm0).abs() + MOM_K * mean.abs()) + MOM_K * dbl * absx
        bound["rv"] = 2 * U32 * ((1 - MOM_K) * dd(rv0).abs() + MOM_K * unb) + MOM_K * dvar * (count / max(count - 1.0, 1.0))
    return {k: v.numpy() for k, v in ref.items()}, {k: v.numpy() for k, v in bound.items()}


def _check_stats(tag, stat, bn, ref, bound, C):
    stat = stat.cpu().numpy()
    _close(tag + " mean", stat[:C], ref["mean"], bound["mean"])
    _close(tag + " invstd", stat[C:], ref["inv"], bound["inv"])
    if "rm" in ref:
        _close(tag + " running_mean", bn.running_mean.cpu().numpy(), ref["rm"], bound["rm"])
        _close(tag + " running_var", bn.running_var.cpu().numpy(), ref["rv"], bound["rv"])
        assert int(bn.num_batches_tracked) == 42


# (3, 5, 7): fewer clips than slices, fewer positions than threads; (64, 3, 204): exactly 64 clips; (67, 65, 300): the strided slice loop
# has a remainder; (130, 2, 513): three clips per slice for two slices only, positions beyond two passes of 256; (1, 4, 1): a count of 1
STATS_SHAPES = [(3, 5, 7), (64, 3, 204), (67, 65, 300), (130, 2, 513), (1, 4, 1)]


@pytest.mark.parametrize("Nb,C,P", STATS_SHAPES)
def test_bn2_stats_train_and_from_partials(Nb, C, P):
    """bn2_stats in train mode, and bn2_stats_parts on double partials [rows, C, 2] the test sums from the same data (rows 1 and 7:
    one row; fewer rows than the finishing kernel's 16 slices): stat, running mean, running variance (unbiased, momentum) and the
    batch counter against double statistics.  Bounds: _stats_ref.  The two entry points round the same double values, so they must also
    agree with each other within that bound."""
    from coskad_amd import ops
    x, g = _channel_data(Nb, C, P, seed=Nb + C + P)
    bn = _bn(C, g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    ref, bound = _stats_ref(x, rm0, rv0)
    stat = ops.bn2_stats(x.cuda(), bn, True)
    _check_stats("stats", stat, bn, ref, bound, C)
    x64 = dd(x)
    for rows in (1, 7):
        parts = torch.zeros(rows, C, 2, dtype=torch.float64)
        for r in range(rows):
            parts[r, :, 0] = x64[r::rows].sum((0, 2))
            parts[r, :, 1] = (x64[r::rows] ** 2).sum((0, 2))
        bn2 = _bn(C, g)
        bn2.running_mean.copy_(rm0); bn2.running_var.copy_(rv0)
        stat2 = ops.bn2_stats_parts(parts.cuda(), bn2, Nb * P)
        _check_stats(f"parts{rows}", stat2, bn2, ref, bound, C)
        b = np.concatenate([bound["mean"], bound["inv"]])
        assert np.all(np.abs(stat2.cpu().numpy().astype(np.float64) - stat.cpu().numpy()) <= b)
        assert np.all(np.abs(bn2.running_var.cpu().numpy().astype(np.float64) - bn.running_var.cpu().numpy()) <= bound["rv"])


def test_bn2_stats_constant_channel_has_zero_variance():
    """a channel held at 1000.0: sum and sum of squares are integers below 2^53, so the double variance is exactly 0 (never
    negative), invstd = 1 / sqrt(eps) and the running variance only decays -- all compared exactly"""
    from coskad_amd import ops
    Nb, C, P = 9, 3, 50
    x, g = _channel_data(Nb, C, P, seed=5)
    x[:, 1, :] = 1000.0
    bn = _bn(C, g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    stat = ops.bn2_stats(x.cuda(), bn, True).cpu().numpy()
    assert stat[1] == np.float32(1000.0)
    assert stat[C + 1] == np.float32(1.0 / np.sqrt(EPS_K))
    assert bn.running_var.cpu().numpy()[1] == np.float32((1.0 - MOM_K) * float(rv0[1]))
    assert bn.running_mean.cpu().numpy()[1] == np.float32((1.0 - MOM_K) * float(rm0[1]) + MOM_K * 1000.0)
    ref, bound = _stats_ref(x, rm0, rv0)
    keep = np.array([0, 2])
    _close("const mean", stat[:C][keep], ref["mean"][keep], bound["mean"][keep])
    _close("const invstd", stat[C:][keep], ref["inv"][keep], bound["inv"][keep])


def test_bn2_stats_without_running_buffers():
    """track_running_stats=False: null running buffers and counter; the statistics alone"""
    from coskad_amd import ops
    Nb, C, P = 6, 4, 33
    x, g = _channel_data(Nb, C, P, seed=8)
    bn = _bn(C, g, track=False)
    assert bn.running_mean is None and bn.num_batches_tracked is None
    ref, bound = _stats_ref(x, None, None)
    _check_stats("norunning", ops.bn2_stats(x.cuda(), bn, True), bn, ref, bound, C)


def test_bn2_stats_eval_reads_the_running_buffers_and_writes_nothing():
    """eval mode: stat[:C] is the running mean bit for bit; stat[C:] = 1.f / sqrtf(rvar + eps) in float32 -- an add (whose error the
    square root halves), a square root and a division, the latter two counted at 2 U32 each: k = 5 on M = invstd.  Buffers and
    counter are compared bitwise before and after."""
    from coskad_amd import ops
    Nb, C, P = 5, 7, 20
    x, g = _channel_data(Nb, C, P, seed=9)
    bn = _bn(C, g)
    before = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    stat = ops.bn2_stats(x.cuda(), bn, False).cpu()
    assert torch.equal(stat[:C].view(torch.int32), before[0].cpu().view(torch.int32))
    inv = 1.0 / torch.sqrt(dd(before[1]) + EPS_K)
    _close("eval invstd", stat[C:].numpy(), inv.numpy(), 5 * U32 * inv.numpy())
    for a, b in zip((bn.running_mean, bn.running_var), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(bn.num_batches_tracked, before[2])


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("seed", R.DROP_SEEDS)
def test_dropout_mask_is_the_restated_hash(p, seed):
    """n = 70 000: element indices beyond 65536 and a last block that is partly filled (not a multiple of 256); compared exactly with
    kernel_refs.drop_mask_twin (Python integers masked to 64 bits).  One seed is above 2^32: the 64-bit parameter arrives whole."""
    from coskad_amd import ops
    n = 70_000
    got = ops.dropout_mask((n,), p, seed, "cuda").cpu().numpy()
    want = R.drop_mask_twin(n, p, seed)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert set(np.unique(got)) <= {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(p))}


# ---- apply + backward ----------------------------------------------------------------------------------------------------------------------

K_U, K_OUT = 9, 10


def _branch_terms(Cx, gam, beta, mean, inv, m):
    s = (gam * inv).abs()
    return m * (s[None, :, None] * Cx.abs() + (beta.abs() + s * mean.abs())[None, :, None])


def _bwd_branch_bounds(Cx, mean, inv, gam, mdu, kd, kink, n, training):
    """bounds of one BatchNorm branch of bn2_bwd: dC [N, C, P], dgamma [C], dbeta [C].

    k_bwd_part sums, in double, s0 = sum m du and sduc = sum (m du) C with du = g or a g (one rounding) and m du (one more):
    err(s0) <= 2 U32 S0, S0 = sum |m du|.  k_bwd_final forms sxh = (sduc - mean s0) invstd from the float32 mean and invstd (one
    rounding each against the double reference): err(sxh) <= 4 U32 Mg, Mg = sum |m du| (|C| + |mean|) invstd.  dbeta = (float) s0 and
    dgamma = (float) sxh add one rounding.  Every left-out element (kink) may flip du by (1 - a)|g|, which widens err(s0) by
    m (1 - a)|g| and err(sxh) by m (1 - a)|g| (|C| + |mean|) invstd.
    dC = fma(k0, m du, fma(k1, C, k2)), k0 = f = gamma invstd, k1 = -f invstd sxh / n, k2 = -f s0 / n + f invstd mean sxh / n, each
    coefficient formed in double and rounded once.  Terms: A = f |m du| (invstd, k0, du, m du, outer fma: 5 roundings);
    B = f S0 / n (invstd, k2, two fma: 4, + f err(s0) / n); Cc = f invstd (|C| + |mean|) Mg / n (invstd twice, the mean of k2, k1 / k2,
    two fma: 6, + f invstd (|C| + |mean|) err(sxh) / n).  Bound: 6 U32 (A + B + Cc) + the two carried errors; in eval mode k1 = k2 = 0
    and only A is left."""
    cm = Cx.abs() + mean.abs()[None, :, None]
    S0 = mdu.sum((0, 2))
    Mg = (mdu * cm).sum((0, 2)) * inv
    ks0 = (kink * kd).sum((0, 2))
    ksx = (kink * kd * cm).sum((0, 2)) * inv
    dbl = (n + 8) * U64
    err_s0 = (2 * U32 + dbl) * S0 + ks0
    err_sx = (4 * U32 + 2 * dbl) * Mg + ksx
    f = (gam * inv).abs()
    A = f[None, :, None] * mdu
    if training:
        B = (f * S0 / n)[None, :, None]
        Cc = (f * inv * Mg / n)[None, :, None] * cm
        bd = 6 * U32 * (A + B + Cc) + (f * err_s0 / n)[None, :, None] + (f * inv * err_sx / n)[None, :, None] * cm
    else:
        bd = 6 * U32 * A
    return bd, err_sx + U32 * Mg, err_s0 + U32 * S0


def _apply_case(Nb, C, P, residual_bn, training, drop_p, mask_fn, a=0.1):
    """inputs of one apply / backward case, the double reference with autograd's gradients, M of u, err(u) and the kink elements;
    mask_fn(shape, p, seed) -> float32 CPU mask (the device's in the GPU test, the Python twin in test_kernel_refs_host.py)"""
    seed = R.bn2_case_seed(Nb, C, P, residual_bn, training, drop_p)
    Ct, g = _channel_data(Nb, C, P, seed)
    Cr = torch.randn(Nb, C, P, generator=g) * 0.8 + 0.3
    dOut = (torch.randn(Nb, C, P, generator=g) + 0.25 * Ct).contiguous()
    par = {k: torch.randn(C, generator=g) for k in ("gt", "bt", "gr", "br")}
    par["gt"] += 1.5 * torch.sign(par["gt"])
    run = {"mt": torch.randn(C, generator=g), "vt": torch.rand(C, generator=g) + 0.5, "mr": torch.randn(C, generator=g),
           "vr": torch.rand(C, generator=g) + 0.5}
    slope = torch.tensor([a])
    drop_seed = (1 << 33) + seed
    mask = mask_fn((Nb, C, P), drop_p, drop_seed) if drop_p > 0 else None
    leaves = {k: dd(v).requires_grad_(True) for k, v in dict(Ct=Ct, Cr=Cr, slope=slope, **par).items()}
    t = dict(gamma=leaves["gt"], beta=leaves["bt"], running_mean=dd(run["mt"]), running_var=dd(run["vt"]))
    r = dict(gamma=leaves["gr"], beta=leaves["br"], running_mean=dd(run["mr"]), running_var=dd(run["vr"])) if residual_bn else None
    out_ref, u_ref, (mean_t, inv_t), sr = R.bn2_block(leaves["Ct"], leaves["Cr"], t, r, leaves["slope"], EPS_K, training,
                                                       None if mask is None else dd(mask))
    names = ["Ct", "Cr", "gt", "bt", "slope"] + (["gr", "br"] if residual_bn else [])
    grads = dict(zip(names, torch.autograd.grad(out_ref, [leaves[k] for k in names], dd(dOut))))
    mean_t, inv_t, u_ref, out_ref = mean_t.detach(), inv_t.detach(), u_ref.detach(), out_ref.detach()
    sr = (sr[0].detach(), sr[1].detach()) if residual_bn else None
    m = dd(mask) if mask is not None else torch.ones_like(u_ref)
    Mu = _branch_terms(dd(Ct), dd(par["gt"]), dd(par["bt"]), mean_t, inv_t, m)
    Mu = Mu + (_branch_terms(dd(Cr), dd(par["gr"]), dd(par["br"]), sr[0], sr[1], torch.ones_like(m)) if residual_bn else dd(Cr).abs())
    errU = K_U * U32 * Mu
    return dict(Ct=Ct, Cr=Cr, dOut=dOut, par=par, slope=slope, mask=mask, drop_seed=drop_seed, out_ref=out_ref, u_ref=u_ref,
                mean_t=mean_t, inv_t=inv_t, sr=sr, grads=grads, Mu=Mu, errU=errU, kink=u_ref.abs() <= errU)


# (5, 3, 7): small, ragged; (67, 65, 204): the strided slice loop with a remainder; (257, 256, 4): Nb C = 65792 rows, above the
# 65536-block cap: the grid-stride row loop runs (263 k floats)
APPLY_SHAPES = [(5, 3, 7), (67, 65, 204), (257, 256, 4)]


@pytest.mark.parametrize("Nb,C,P", APPLY_SHAPES)
@pytest.mark.parametrize("residual_bn", [True, False])
@pytest.mark.parametrize("training,drop_p", [(True, 0.0), (True, 0.25), (False, 0.0)])
def test_bn2_apply_and_bwd(Nb, C, P, residual_bn, training, drop_p):
    """out = PReLU(m BN_t(Ct) + BN_r(Cr)) and its backward against kernel_refs.bn2_block in double with autograd's gradients.  The
    kernels get `stat` from the double reference rounded to float32 (the batch statistics in train mode, the running ones in eval
    mode), so bn2_bwd is tested on its own; slope 0.1, random gamma / beta; the mask is coskad_dropout_mask_f32's, applied inside the
    reference.

    u = m fma(st, Ct, ht) + fma(sr, Cr, hr), st = gamma invstd, ht = beta - st mean.  Longest chain, the term st mean: invstd and
    mean rounded to float32 (2), st (1), st mean (1), ht (1), fma (1), m . (1), the add (1) = 8, one spare: K_U = 9; the PReLU's
    a u adds one: K_OUT = 10.  M = m (|st Ct| + |beta| + |st mean|) + the same of the residual branch (|Cr| for the identity).
    The kink: where |u_ref| <= K_U U32 M the float32 u may take the other PReLU branch; `out` is continuous there and compared
    everywhere, dCt / dCr leave those elements out, the reductions are widened by what they may contribute (_bwd_branch_bounds), and
    their share must stay <= 1e-3.  dslope = sum g u [u < 0] in double over the float32 u: sum_{u_ref < 0} |g| err(u) +
    2 sum_kink |g| err(u) + (U32 + the double term) sum |g u|."""
    from coskad_amd import ops
    a = 0.1
    k = _apply_case(Nb, C, P, residual_bn, training, drop_p, lambda shape, p, seed: ops.dropout_mask(shape, p, seed, "cuda").cpu())
    Ct, Cr, dOut, par, slope, mask, drop_seed = k["Ct"], k["Cr"], k["dOut"], k["par"], k["slope"], k["mask"], k["drop_seed"]
    out_ref, u_ref, mean_t, inv_t, sr, grads, Mu, errU, kink = (k[n] for n in ("out_ref", "u_ref", "mean_t", "inv_t", "sr", "grads", "Mu",
                                                                               "errU", "kink"))
    if mask is not None:
        assert 0.6 < float((mask > 0).float().mean()) < 0.9

    # the kernels
    stat_t = torch.cat([mean_t, inv_t]).float().cuda()
    stat_r = torch.cat(sr).float().cuda() if residual_bn else None
    dev = {k: v.cuda() for k, v in dict(Ct=Ct, Cr=Cr, dOut=dOut, slope=slope, **par).items()}
    gr, br = (dev["gr"], dev["br"]) if residual_bn else (None, None)
    out = ops.bn2_apply_prelu(dev["Ct"], dev["Cr"], stat_t, dev["gt"], dev["bt"], stat_r, gr, br, dev["slope"], drop_p, drop_seed)
    dCt, dCr, dgt, dbt, dgr, dbr, dslope = ops.bn2_bwd(dev["Ct"], dev["Cr"], dev["dOut"], stat_t, dev["gt"], dev["bt"], stat_r, gr, br,
                                                       dev["slope"], training, drop_p, drop_seed)
    torch.cuda.synchronize()

    # bounds
    Ct64, Cr64, g64 = dd(Ct), dd(Cr), dd(dOut)
    m = dd(mask) if mask is not None else torch.ones_like(Ct64)
    if residual_bn:
        mean_r, inv_r = sr
    share = float(kink.double().mean())
    print(f"RATIO kink-share/1e-3 {share / 1e-3:.3f}")
    assert share <= 1e-3
    keep = (~kink).numpy()
    tag = f"{'bn' if residual_bn else 'id'}/{'train' if training else 'eval'}/p{drop_p}"
    _close(tag + " out", out.cpu().numpy(), out_ref.numpy(), (K_OUT * U32 * Mu).numpy())

    a_k = R.f32(a)
    du = torch.where(u_ref > 0, g64, a_k * g64).abs()
    kd = (1.0 - a_k) * g64.abs()
    n = Nb * P
    bd, bg, bb = _bwd_branch_bounds(Ct64, mean_t, inv_t, dd(par["gt"]), m * du, m * kd, kink, n, training)
    _close(tag + " dCt", dCt.cpu().numpy(), grads["Ct"].numpy(), bd.numpy(), keep)
    _close(tag + " dgamma_t", dgt.cpu().numpy(), grads["gt"].numpy(), bg.numpy())
    _close(tag + " dbeta_t", dbt.cpu().numpy(), grads["bt"].numpy(), bb.numpy())
    if residual_bn:
        bd, bg, bb = _bwd_branch_bounds(Cr64, mean_r, inv_r, dd(par["gr"]), du, kd, kink, n, training)
        _close(tag + " dCr", dCr.cpu().numpy(), grads["Cr"].numpy(), bd.numpy(), keep)
        _close(tag + " dgamma_r", dgr.cpu().numpy(), grads["gr"].numpy(), bg.numpy())
        _close(tag + " dbeta_r", dbr.cpu().numpy(), grads["br"].numpy(), bb.numpy())
    else:
        assert dgr is None and dbr is None
        g32 = dOut.numpy()
        gated = np.where(u_ref.numpy() > 0, g32, np.float32(a) * g32)          # float32: the PReLU-gated dOut, bit for bit
        assert gated.dtype == np.float32 and np.array_equal(dCr.cpu().numpy()[keep], gated[keep])
        _close(tag + " dCr", dCr.cpu().numpy(), grads["Cr"].numpy(), (U32 * du).numpy(), keep)
    gu = g64.abs() * u_ref.abs()
    b_slope = ((g64.abs() * errU)[u_ref < 0].sum() + 2 * (g64.abs() * errU)[kink].sum()
               + (U32 + (Nb * C * P + 8) * U64) * gu[u_ref < 0].sum())
    _close(tag + " dslope", dslope.cpu().numpy(), grads["slope"].numpy(), np.full(1, float(b_slope)))
