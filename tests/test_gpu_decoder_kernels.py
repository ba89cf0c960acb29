"""Kernel-level checks of the stand-alone kernels that exist only for the decoder models (autoencoder, spherical VAE, `mlp` projector):
csrc/rev_btlnk.hip at latent 8 / 16 (k_rev_fwd, k_rev_dw, k_rev_dw_sum, k_rev_dz), csrc/lowrank_fold.hip (k_fold_fwd, k_fold_bwd) and
both kernel sets of csrc/mlp_head.hip, called through the C entry points with guard bands around every output and workspaces the
test allocates itself and fills with NaN, against the float64 restatements of kernel_refs.py (rev_btlnk, fold, mlp_head) with
autograd's gradients.

Every bound is  k * U32 * M  (+ (count + 8) * U64 * M for what a kernel sums in double): M the double sum of the absolute values of
the element's terms, k the float32 roundings on the longest chain a term passes through, read from the kernel -- the functions k_* and
*_bounds below carry the derivations.  Where a float32 value that is itself off by a bound e feeds a later expression, e is carried
through that expression's partial derivative (first order), as written out in the docstrings.  The library is built with
-ffp-contract=off: every add and multiply written in a kernel rounds once, and so does every fmaf.  The chain lengths come from the
plan restatements of kernel_refs.py, which test_kernel_refs_host.py holds against the library's own size queries.  Nothing is fitted
to the kernels' output.  Each check prints `RATIO <name> <largest error / bound>` (DESIGN.md 6.1 records a run)."""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_refs import U32, U64, ceil_div, dd
from test_gpu_head_rides import _same_bits
from test_gpu_wide_kernels import _close
from test_gpu_wide_latent import GUARD, SENT, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

PRIOR = 0.5                       # what `accumulate` adds onto
NAN = float("nan")
ERR_ARG, ERR_SHAPE = -1, -2       # COSKAD_ERR_ARG, COSKAD_ERR_SHAPE (csrc/common.h)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------

def _lib():
    from coskad_amd import _lib as L
    return L


def _stream():
    from coskad_amd import ops
    return ops._stream()


def _out(shape, fill, dtype=torch.float32):
    """a guarded output (SENT on both sides) holding `fill` -> (parent, view); the view is 16-byte aligned"""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        buf, v = _guarded(n)
    else:
        buf = torch.full((n + 2 * GUARD,), SENT, device="cuda", dtype=dtype)
        v = buf[GUARD:GUARD + n]
    v.fill_(fill)
    return buf, v.view(*shape)


def _intact(bufs, tag):
    for k, (buf, _) in bufs.items():
        _guards_intact(buf, f"{tag} {k}")


def _scratch(nfloats):
    """a float workspace handed over as NaN: a partial the kernels do not write is a NaN in whatever sums it"""
    return torch.full((int(nfloats) + 2,), NAN, dtype=torch.float32, device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ======================================================================================================================================
# A. rev_btlnk, latent 8 and 16
# ======================================================================================================================================

REV_LS = (8, 16)
# one thread; under one column block; the `n >= N` return inside a second block and a second k_rev_dz stride of one float4; 32 x 204
REV_NS = (4, 816, 1028, 6528)
# k_rev_dz's CB = 4 / 2 with every remainder; rb::slices 1 -> 2 -> 3 -> 63 -> 64 with wholly empty trailing slices at 1030; the
# forward's 1 / 4 / slices branches on both sides of 64 and 1024  (test_kernel_refs_host.py asserts each from the restatement)
REV_BS = (1, 2, 3, 5, 15, 16, 17, 33, 63, 64, 65, 1023, 1024, 1030)
REV_BMAX = max(REV_BS)
REV_PROD = (450, 38400, 16)       # a production-range batch: 27 slices, strictly between the clamps


def k_rev_h(L):
    """k_rev_fwd: o = bias (or 0.f), then one fmaf per latent: L roundings"""
    return L


def k_rev_dz(N, acc):
    """k_rev_dz: a thread's accumulator takes four nested fmaf per stride of 1024 columns (4 ceil(N / 1024)), wave_sum's six butterfly
    adds (6), the four waves as (s0 + s1) + (s2 + s3) (2), and *out + s under dz_accumulate (1)"""
    return 4 * ceil_div(N, 1024) + 6 + 2 + int(acc)


def k_rev_dw(chunk, acc):
    """k_rev_dw: one fmaf per clip of the slice from 0.f (chunk); k_rev_dw_sum adds the S slices in double, converts (1), and adds onto
    the prior under `accumulate` (1)"""
    return chunk + 1 + int(acc)


def k_rev_db(chunk, acc):
    """column L of the same table: acc += g per clip, the first onto 0.f exact (chunk - 1), the conversion (1), the accumulate (1)"""
    return chunk - 1 + 1 + int(acc)


def _bd(k, M, count=None):
    return (k * U32 + (0.0 if count is None else (count + 8) * U64)) * M


def _rev_fwd(dev, bias, B, N, L):
    bufs = {"H": _out((B, N), NAN)}
    _lib().call("coskad_rev_btlnk_fwd_f32", dev["z"], dev["W"], dev["b"] if bias else None, bufs["H"][1], B, N, L, _stream())
    _intact(bufs, "rev fwd")
    return bufs["H"][1]


def _rev_bwd(dev, B, N, L, dz_acc=False, acc=False, with_db=True):
    """coskad_rev_btlnk_bwd_f32 on the leading B clips: dz onto NaN or onto the prior dz0, dW / db onto NaN or PRIOR, the workspace NaN"""
    lib = _lib()
    fill = PRIOR if acc else NAN
    bufs = {"dz": _out((B, L), NAN), "dW": _out((N, L), fill), "db": _out((N,), fill)}
    if dz_acc:
        bufs["dz"][1].copy_(dev["dz0"][:B])
    ws = _scratch(lib.lib().coskad_rev_btlnk_ws_floats(B, N, L))
    lib.call("coskad_rev_btlnk_bwd_f32", dev["dH"], dev["z"], dev["W"], bufs["dz"][1], 1 if dz_acc else 0, bufs["dW"][1],
             bufs["db"][1] if with_db else None, 1 if acc else 0, ws, B, N, L, _stream())
    _intact(bufs, "rev bwd")
    return {k: v[1] for k, v in bufs.items()}


def _rev_param_ref(d, B):
    """double dW / db of the leading B clips and their M"""
    dH, z = dd(d["dH"][:B]), dd(d["z"][:B])
    return (dict(dW=_np(dH.T @ z), db=_np(dH.sum(0))), dict(dW=_np(dH.abs().T @ z.abs()), db=_np(dH.abs().sum(0))))


def _rev_check_params(tag, out, ref, M, B, N, acc):
    S = R.rev_slices(B, N)
    chunk = ceil_div(B, S)
    prior = PRIOR if acc else 0.0
    _close(f"{tag} dW", _np(out["dW"]), ref["dW"] + prior, _bd(k_rev_dw(chunk, acc), M["dW"] + prior, S))
    _close(f"{tag} db", _np(out["db"]), ref["db"] + prior, _bd(k_rev_db(chunk, acc), M["db"] + prior, S))


@pytest.mark.parametrize("L", REV_LS)
@pytest.mark.parametrize("N", REV_NS)
def test_rev_btlnk(N, L):
    """coskad_rev_btlnk_fwd_f32 / coskad_rev_btlnk_bwd_f32 at every B of REV_BS on the leading clips of one input set.
    Forward: H of the largest batch within k_rev_h U32 M (M = |z| |W|^T + |b|) with and without a bias, a repeat bit-equal, and H of
    every smaller batch bit-equal to its leading rows -- a clip's row does not depend on which of the three slice branches it ran in.
    Backward: dz of the largest batch within k_rev_dz U32 M (M = |dH| |W|, + |prior| when added onto one), every smaller batch
    bit-equal to the leading rows in both modes; dW / db of every batch within k_rev_dw / k_rev_db with chunk = ceil(B / S), the S
    slices summed in double, overwritten onto NaN and accumulated onto PRIOR; a repeat call bit-equal; db absent with dW and dz
    bit-equal to the full call.  The workspace arrives as NaN, so a slice row nobody wrote shows in dW."""
    d = R.rev_inputs(REV_BMAX, N, L, seed=31 * N + L)
    dev = {k: v.cuda() for k, v in d.items()}
    z, W, dH = dd(d["z"]), dd(d["W"]), dd(d["dH"])
    tag = f"rev N={N} L={L}"
    # forward
    for bias in (True, False):
        b = dd(d["b"]) if bias else None
        Href = R.rev_btlnk(z, W, b)
        M = z.abs() @ W.abs().T + (b.abs() if bias else 0.0)
        full = _rev_fwd(dev, bias, REV_BMAX, N, L)
        _close(f"{tag} H bias={bias}", _np(full), _np(Href), k_rev_h(L) * U32 * _np(M))
        assert _same_bits(_rev_fwd(dev, bias, REV_BMAX, N, L), full), ("repeat", bias)
        for B in REV_BS[:-1]:
            assert _same_bits(_rev_fwd(dev, bias, B, N, L), full[:B]), ("H batch independence", bias, B)
    # backward
    dzref, Mdz = dH @ W, dH.abs() @ W.abs()
    dz0 = dd(d["dz0"])
    full = _rev_bwd(dev, REV_BMAX, N, L)
    fullacc = _rev_bwd(dev, REV_BMAX, N, L, dz_acc=True, acc=True)
    _close(f"{tag} dz", _np(full["dz"]), _np(dzref), k_rev_dz(N, False) * U32 * _np(Mdz))
    _close(f"{tag} dz onto a prior", _np(fullacc["dz"]), _np(dzref + dz0), k_rev_dz(N, True) * U32 * _np(Mdz + dz0.abs()))
    for B in REV_BS:
        ref, M = _rev_param_ref(d, B)
        out = full if B == REV_BMAX else _rev_bwd(dev, B, N, L)
        assert _same_bits(out["dz"], full["dz"][:B]), ("dz batch independence", B)
        _rev_check_params(f"{tag} B={B}", out, ref, M, B, N, False)
        again = _rev_bwd(dev, B, N, L)
        for q in ("dz", "dW", "db"):
            assert _same_bits(again[q], out[q]), ("repeat", B, q)
        acc = fullacc if B == REV_BMAX else _rev_bwd(dev, B, N, L, dz_acc=True, acc=True)
        assert _same_bits(acc["dz"], fullacc["dz"][:B]), ("dz onto a prior, batch independence", B)
        _rev_check_params(f"{tag} B={B} accumulate", acc, ref, M, B, N, True)
        nodb = _rev_bwd(dev, B, N, L, with_db=False)
        assert _same_bits(nodb["dW"], out["dW"]) and _same_bits(nodb["dz"], out["dz"]), ("without db", B)
        assert _all_nan(nodb["db"]), "db written though absent"


def test_rev_btlnk_production_batch():
    """(450, 38400, 16): rb::slices lands strictly between its clamps (27: asserted from the restatement); H with a bias, dz, dW and db
    within the same bounds"""
    B, N, L = REV_PROD
    S = R.rev_slices(B, N)
    assert S == 27 and 16 < S < min(64, B // 16) and R.rev_fwd_slices(B, N) == 4
    d = R.rev_inputs(B, N, L, seed=9)
    dev = {k: v.cuda() for k, v in d.items()}
    z, W, dH, b = dd(d["z"]), dd(d["W"]), dd(d["dH"]), dd(d["b"])
    tag = f"rev {B}x{N}x{L}"
    H = _rev_fwd(dev, True, B, N, L)
    _close(f"{tag} H", _np(H), _np(R.rev_btlnk(z, W, b)), k_rev_h(L) * U32 * _np(z.abs() @ W.abs().T + b.abs()))
    del H
    out = _rev_bwd(dev, B, N, L)
    _close(f"{tag} dz", _np(out["dz"]), _np(dH @ W), k_rev_dz(N, False) * U32 * _np(dH.abs() @ W.abs()))
    ref, M = _rev_param_ref(d, B)
    _rev_check_params(tag, out, ref, M, B, N, False)


def test_rev_btlnk_refusals():
    """the C entry points refuse a dH / H that is not 16-byte aligned (COSKAD_ERR_ARG), N % 4 != 0 and L = 12 (COSKAD_ERR_SHAPE), and
    write nothing"""
    lib = _lib().lib()
    st = _stream()
    B, N, L = 5, 8, 8
    g = torch.Generator().manual_seed(1)
    z, W, b = (torch.randn(s, generator=g).cuda() for s in ((B, 16), (N + 4, 16), (N + 4,)))
    flat = torch.randn(B * (N + 4) + 4, generator=g).cuda()

    def outs():
        return {"H": _out((B * (N + 4) + 4,), NAN), "dz": _out((B, 16), NAN), "dW": _out((N + 4, 16), NAN), "db": _out((N + 4,), NAN)}

    def unwritten(o, what):
        _intact(o, what)
        assert all(_all_nan(v) for _, v in o.values()), what

    ws = _scratch(lib.coskad_rev_btlnk_ws_floats(B, N + 4, 16))
    for Bc, Nc, Lc, off, rc in ((B, N, L, 1, ERR_ARG), (B, N, 16, 3, ERR_ARG), (B, N + 2, L, 0, ERR_SHAPE), (B, N, 12, 0, ERR_SHAPE),
                                (B, N + 1, 12, 0, ERR_SHAPE)):
        o = outs()
        assert lib.coskad_rev_btlnk_fwd_f32(z.data_ptr(), W.data_ptr(), b.data_ptr(), o["H"][1][off:].data_ptr(), Bc, Nc, Lc, st) == rc, \
            ("fwd", Bc, Nc, Lc, off)
        assert lib.coskad_rev_btlnk_bwd_f32(flat[off:].data_ptr(), z.data_ptr(), W.data_ptr(), o["dz"][1].data_ptr(), 0, o["dW"][1].data_ptr(),
                                            o["db"][1].data_ptr(), 0, ws.data_ptr(), Bc, Nc, Lc, st) == rc, ("bwd", Bc, Nc, Lc, off)
        torch.cuda.synchronize()
        unwritten(o, f"refused {Bc}x{Nc}x{Lc} offset {off}")
    assert bool(torch.isnan(ws).all())


# ======================================================================================================================================
# B. lowrank_fold
# ======================================================================================================================================

FOLD_COS = (1, 3, 32)
# one position; one ragged round; exactly one round; one into the second; ragged second rounds; both rounds full
FOLD_TVS = (1, 63, 136, 204, 256, 257, 300, 408, 512)
FOLD_NS = (1, 37)                 # n = 1, TV = 1: n_pos = 1, the `unb = 1` branch
FOLD_MOM = (0.1, 0.3)             # per branch
FOLD_EPS = (1e-5, 1e-3)
NBT0 = 41
# conv bias / running buffers / num_batches_tracked given per branch; Mw, Mb and what the backward keeps do not depend on them
FOLD_CFGS = [dict(cbias=(True, True), run=(True, True), nbt=(True, True)), dict(cbias=(False, True), run=(True, False), nbt=(False, False)),
             dict(cbias=(True, False), run=(False, True), nbt=(False, True)), dict(cbias=(False, False), run=(False, False), nbt=(False, False))]
K9 = R.FOLD_K


def _fold_fwd(dev, Co, TV, n_pos, cfg):
    bufs = {"Mw": _out((Co * TV, K9 - 1), NAN), "Mb": _out((Co * TV,), NAN), "saved": _out((3, 2, Co), NAN, torch.float64),
            "xbar": _out((2, K9, Co), NAN, torch.float64), "xx": _out((2, Co, K9, K9), NAN, torch.float64)}
    run, args = {}, []
    for r in range(2):
        if cfg["run"][r]:
            run[f"rmean{r}"], run[f"rvar{r}"] = _out((Co,), 0.0), _out((Co,), 0.0)
            run[f"rmean{r}"][1].copy_(dev[f"rmean{r}"]); run[f"rvar{r}"][1].copy_(dev[f"rvar{r}"])
        nbt = torch.full((1,), NBT0, dtype=torch.int64, device="cuda") if cfg["nbt"][r] else None
        run[f"nbt{r}"] = nbt
        args += [dev[f"gamma{r}"], dev[f"beta{r}"], dev[f"cbias{r}"] if cfg["cbias"][r] else None,
                 run[f"rmean{r}"][1] if cfg["run"][r] else None, run[f"rvar{r}"][1] if cfg["run"][r] else None, nbt, FOLD_MOM[r], FOLD_EPS[r]]
    _lib().call("coskad_lowrank_fold_fwd_f32", dev["X"], dev["G"], *args, n_pos, bufs["Mw"][1], bufs["Mb"][1], bufs["saved"][1],
                bufs["xbar"][1], bufs["xx"][1], Co, TV, _stream())
    _intact(bufs, "fold fwd")
    _intact({k: v for k, v in run.items() if isinstance(v, tuple)}, "fold fwd")
    out = {k: v[1] for k, v in bufs.items()}
    out.update({k: (v[1] if isinstance(v, tuple) else v) for k, v in run.items()})
    return out


def _fold_bwd(dev, fwd, Co, TV, n_pos):
    bufs = {"dX": _out((2, K9, Co, TV), NAN), "dgamma": _out((2, Co), NAN), "dbeta": _out((Co,), NAN), "dGc": _out((Co, K9, K9), NAN, torch.float64)}
    _lib().call("coskad_lowrank_fold_bwd_f32", dev["X"], dev["G"], dev["dMw"], dev["dMb"], fwd["saved"], fwd["xbar"], fwd["xx"], dev["gamma0"],
                dev["gamma1"], n_pos, bufs["dX"][1], bufs["dgamma"][1], bufs["dbeta"][1], bufs["dGc"][1], Co, TV, _stream())
    _intact(bufs, "fold bwd")
    return {k: v[1] for k, v in bufs.items()}


def fold_case(Co, TV, n):
    """Inputs, the double reference (kernel_refs.fold with autograd, G a leaf per channel) and every bound of one fold case.  No device.

    Forward, all in double in the kernel (TV positions per sum, a tree over the block; products of two float32 are exact in double):
      xbar, xx      (TV + 8) U64 M, M = sum |x|, sum |x_l x_m|
      mean          9 terms G[l, 8] xbar_l and a division on top: e_mean = (TV + 9 + 24) U64 M, M = sum_l |G[l, 8]| sum |x| / n_pos
      E2            81 terms (the off-diagonal G[l, m] + G[m, l] is one more add): e_E2 = (TV + 81 + 24) U64 M
      var           E2 - mean^2, M from the terms of both: e_var = e_E2 + 2 |mean| e_mean + 4 U64 (M_E2 + mean^2).  This is the
                    cancellation: with a constant image 10^3 times the spread M_E2 is 10^6 var.
      istd          (var + eps)^(-1/2): e_istd = istd / (2 (var + eps)) e_var + 4 U64 istd;  a = gamma istd: e_a = |gamma| e_istd + U64 |a|
    Float32 outputs:
      Mw            a_0 x_0 + a_1 x_1: (float) a (1), the product (1), the add (1): 3 U32 sum_r |a_r x_r| + sum_r e_a |x_r|
      Mb            ... + sh, sh = (float)(sum_r beta_r - a_r mean_r) (1) and a second add: 4 U32 (sum_r |a_r x_r| + |beta_r| + |a_r mean_r|)
                    + sum_r (e_a (|x_r| + |mean_r|) + |a_r| e_mean)
      running mean  (1.f - mom) rm + mom ((float) mean + cbias): 4 roundings on the longest term: 4 U32 ((1 - mom) |rm| + mom (|mean| +
                    |cbias|)) + mom e_mean;   running variance (1.f - mom) rv + mom (float)(var unb): 4 U32 M + mom unb e_var
    Backward (S1 = sum dMb, P_r = sum_p sum_l dM_l x_rl, each position's nine products one float32 fmaf chain, the positions in double):
      da = P - mean S1:  e_da = (9 U32 + (TV + 8) U64) M_P + |mean| (TV + 8) U64 sum |dMb| + |S1| e_mean + 4 U64 M_da
      dgamma = (float)(da istd): istd e_da + |da| e_istd + U32 |dgamma|;   dbeta = (float) S1: U32 |S1| + (TV + 8) U64 sum |dMb|
      dvar = -da gamma istd^3 / 2:  e_dvar = |gamma| istd^3 e_da / 2 + 3 |dvar| e_istd / istd + 8 U64 |dvar|
      dmean = -a S1 - 2 mean dvar:  e_dmean = |a| (TV + 8) U64 sum |dMb| + e_a |S1| + 2 |mean| e_dvar + 2 |dvar| e_mean + 8 U64 (..)
      dGc = sum_r (dvar xx + [m = 8] dmean xbar) / n_pos: a float64 output, but dvar carries da's float32 chain (the 9 U32 above), so it
            cannot be held to U64 alone: e = sum_r (e_dvar |xx| + |dvar| e_xx + [m = 8] (e_dmean |xbar| + |dmean| e_xbar)) / n_pos + 8 U64 M
      dX = cf0 dM_l + cf1 G32[l, 8] + cf2 sum_m G32[l, m] x_m, cf = (float)(a, dmean / n_pos, 2 dvar / n_pos), G32 = (float) G: the last
            term passes cf2 (1), G32 (1), nine fmaf (9), the product (1) and one add (1): 13 U32 M_dX + e_a |dM| + e_dmean |G[l, 8]| / n_pos
            + 2 e_dvar sum_m |G[l, m] x_m| / n_pos."""
    d = R.fold_inputs(Co, TV, n, seed=1000 * Co + 10 * TV + n)
    n_pos = d["n_pos"]
    G = d["G"]
    leaf = lambda t: dd(t).clone().requires_grad_(True)
    X, Gc = leaf(d["X"]), G[None].expand(Co, K9, K9).clone().requires_grad_(True)
    gam, bet = [leaf(d["gamma0"]), leaf(d["gamma1"])], [leaf(d["beta0"]), leaf(d["beta1"])]
    f = R.fold(X, Gc, gam, bet, FOLD_EPS, n_pos)
    dMw, dMb = dd(d["dMw"]), dd(d["dMb"])
    loss = (f["Mw"].reshape(Co * TV, K9 - 1) * dMw).sum() + (f["Mb"].reshape(Co * TV) * dMb).sum()
    gX, gG, gg0, gg1, gb0, gb1 = torch.autograd.grad(loss, [X, Gc] + gam + bet)
    f = {k: v.detach() for k, v in f.items()}
    X = X.detach()
    ref = dict(Mw=f["Mw"].reshape(Co * TV, K9 - 1), Mb=f["Mb"].reshape(Co * TV), saved=torch.stack([f["mean"], f["istd"], f["a"]]),
               xbar=f["xbar"], xx=f["xx"], dX=gX, dGc=gG, dgamma=torch.stack([gg0, gg1]), dbeta=gb0)
    assert torch.equal(gb0, gb1)
    # ---- bounds
    gamma, beta = torch.stack([dd(d["gamma0"]), dd(d["gamma1"])]), torch.stack([dd(d["beta0"]), dd(d["beta1"])])
    epsv = torch.tensor([R.f32(e) for e in FOLD_EPS], dtype=torch.float64)[:, None]
    aX = X.abs()
    dTV = (TV + 8) * U64
    Mxbar, Mxx = aX.sum(-1), torch.einsum("rlcp,rmcp->rclm", aX, aX)
    mean, var, istd, a = f["mean"], f["var"], f["istd"], f["a"]
    e_xbar, e_xx = dTV * Mxbar, dTV * Mxx
    e_mean = (TV + K9 + 24) * U64 * torch.einsum("l,rlc->rc", G[:, K9 - 1].abs(), Mxbar) / n_pos
    ME2 = torch.einsum("lm,rclm->rc", G.abs(), Mxx) / n_pos
    e_var = (TV + K9 * K9 + 24) * U64 * ME2 + 2 * mean.abs() * e_mean + 4 * U64 * (ME2 + mean * mean)
    e_istd = 0.5 * istd / (var + epsv) * e_var + 4 * U64 * istd
    e_a = gamma.abs() * e_istd + U64 * a.abs()
    bound = dict(xbar=e_xbar, xx=e_xx, saved=torch.stack([e_mean, e_istd, e_a]))
    MM = torch.einsum("rc,rlcp->cpl", a.abs(), aX)
    eM = torch.einsum("rc,rlcp->cpl", e_a, aX)
    bound["Mw"] = (3 * U32 * MM[:, :, :K9 - 1] + eM[:, :, :K9 - 1]).reshape(Co * TV, K9 - 1)
    shM = (beta.abs() + (a * mean).abs()).sum(0)[:, None]
    she = (e_a * mean.abs() + a.abs() * e_mean).sum(0)[:, None]
    bound["Mb"] = (4 * U32 * (MM[:, :, K9 - 1] + shM) + eM[:, :, K9 - 1] + she).reshape(Co * TV)
    unb = n_pos / (n_pos - 1.0) if n_pos > 1 else 1.0
    run = {}
    for r in range(2):
        mom = R.f32(FOLD_MOM[r])
        rm0, rv0, cb = dd(d[f"rmean{r}"]), dd(d[f"rvar{r}"]), dd(d[f"cbias{r}"])
        for with_bias in (True, False):
            rm, rv = R.fold_running(mean[r], var[r], n_pos, cb if with_bias else None, rm0, rv0, FOLD_MOM[r])
            brm = 4 * U32 * ((1 - mom) * rm0.abs() + mom * (mean[r].abs() + (cb.abs() if with_bias else 0.0))) + mom * e_mean[r]
            brv = 4 * U32 * ((1 - mom) * rv0.abs() + mom * var[r] * unb) + mom * unb * e_var[r]
            run[(r, with_bias)] = (rm, rv, brm, brv)
    # backward
    dM = torch.cat([dMw.view(Co, TV, K9 - 1), dMb.view(Co, TV, 1)], -1)                  # [Co, TV, 9]
    S1, MS1 = dMb.view(Co, TV).sum(1), dMb.view(Co, TV).abs().sum(1)
    P, MP = torch.einsum("cpl,rlcp->rc", dM, X), torch.einsum("cpl,rlcp->rc", dM.abs(), aX)
    da, Mda = P - mean * S1, MP + mean.abs() * MS1
    e_da = (K9 * U32 + dTV) * MP + mean.abs() * dTV * MS1 + S1.abs() * e_mean + 4 * U64 * Mda
    dgam = da * istd
    bound["dgamma"] = istd * e_da + da.abs() * e_istd + U32 * dgam.abs()
    bound["dbeta"] = U32 * S1.abs() + dTV * MS1
    dvar = -0.5 * da * gamma * istd ** 3
    dmean = -a * S1 - 2 * mean * dvar
    xb = f["xbar"].permute(0, 2, 1)                                                      # [2, Co, 9]
    w4 = lambda t: t[:, :, None, None]

    def dG_chain(e_da):
        """e_dvar, e_dmean and dGc's bound from a given bound of da"""
        e_dvar = 0.5 * gamma.abs() * istd ** 3 * e_da + 3 * dvar.abs() * e_istd / istd + 8 * U64 * dvar.abs()
        e_dmean = (a.abs() * dTV * MS1 + e_a * S1.abs() + 2 * mean.abs() * e_dvar + 2 * dvar.abs() * e_mean
                   + 8 * U64 * ((a * S1).abs() + 2 * (mean * dvar).abs()))
        eG = (w4(e_dvar) * f["xx"].abs() + w4(dvar.abs()) * e_xx + 8 * U64 * w4(dvar.abs()) * f["xx"].abs()).sum(0)
        eG[:, :, K9 - 1] += (e_dmean[:, :, None] * xb.abs() + dmean.abs()[:, :, None] * e_xbar.permute(0, 2, 1)
                             + 8 * U64 * dmean.abs()[:, :, None] * xb.abs()).sum(0)
        return e_dvar, e_dmean, eG / n_pos

    e_dvar, e_dmean, bound["dGc"] = dG_chain(e_da)
    dGc_u64 = dG_chain(e_da - K9 * U32 * MP)[2]          # what the bound would be without da's float32 chain: printed, not asserted
    aGX = torch.einsum("lm,rmcp->rlcp", G.abs(), aX)
    gl8 = G[:, K9 - 1].abs()[None, :, None, None]
    dMr = dM.permute(2, 0, 1)[None].abs()                                                 # [1, 9, Co, TV]
    bc = lambda t: t[:, None, :, None]
    MdX = bc(a.abs()) * dMr + bc(dmean.abs()) / n_pos * gl8 + 2 * bc(dvar.abs()) / n_pos * aGX
    bound["dX"] = 13 * U32 * MdX + bc(e_a) * dMr + bc(e_dmean) / n_pos * gl8 + 2 * bc(e_dvar) / n_pos * aGX
    return dict(d=d, ref={k: _np(v) for k, v in ref.items()}, bound={k: _np(v) for k, v in bound.items()}, run=run, var=var, istd=istd,
                dGc_u64=_np(dGc_u64))


@pytest.mark.parametrize("Co", FOLD_COS)
@pytest.mark.parametrize("TV", FOLD_TVS)
def test_lowrank_fold(TV, Co):
    """coskad_lowrank_fold_fwd_f32 / _bwd_f32 for n in FOLD_NS clips, per-branch momentum and eps, against kernel_refs.fold (held to
    nn.BatchNorm2d on the expanded layer by test_kernel_refs_host.py): Mw, Mb; saved (mean, istd, a), xbar, xx in double, xx symmetric
    bit for bit; the running statistics and num_batches_tracked under every configuration of FOLD_CFGS (conv biases, running buffers
    and counters given or absent per branch), Mw / Mb / saved / xbar / xx bit-equal across them; a repeat on fresh running buffers
    bit-equal; dX, dgamma, dbeta, dGc, the backward repeated bit-equal.  Bounds: fold_case.  Channel 1 (Co >= 2) has branch 0 all zero:
    the reference variance is exactly 0 and the kernel's istd is 1 / sqrt(eps) (its bound there is 4 U64 istd); the last channel of
    Co >= 3 has a constant image 10^3 times its spread."""
    lib = _lib().lib()
    assert lib.coskad_lowrank_fold_ok(K9 - 1, TV) == 1
    for n in FOLD_NS:
        c = fold_case(Co, TV, n)
        d, ref, bound = c["d"], c["ref"], c["bound"]
        n_pos = d["n_pos"]
        dev = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
        tag = f"fold Co={Co} TV={TV} n={n}"
        if Co >= 2:
            assert float(c["var"][0, 1]) == 0.0 and bound["saved"][1, 0, 1] <= 5 * U64 * float(c["istd"][0, 1])
            assert float(c["istd"][0, 1]) == pytest.approx(1.0 / np.sqrt(R.f32(FOLD_EPS[0])), rel=1e-15)
        first = None
        for cfg in FOLD_CFGS:
            out = _fold_fwd(dev, Co, TV, n_pos, cfg)
            if first is None:
                first = out
                for q in ("Mw", "Mb", "saved", "xbar", "xx"):
                    _close(f"{tag} {q}", _np(out[q]), ref[q], bound[q])
                for nm, i in (("mean", 0), ("istd", 1), ("a", 2)):
                    _close(f"{tag} saved.{nm}", _np(out["saved"][i]), ref["saved"][i], bound["saved"][i])
                assert _same_bits(out["xx"], out["xx"].transpose(2, 3).contiguous()), "xx not symmetric"
                again = _fold_fwd(dev, Co, TV, n_pos, cfg)
                for q in ("Mw", "Mb", "saved", "xbar", "xx", "rmean0", "rvar0", "rmean1", "rvar1"):
                    assert _same_bits(again[q], out[q]), ("repeat", q)
            else:
                for q in ("Mw", "Mb", "saved", "xbar", "xx"):
                    assert _same_bits(out[q], first[q]), (cfg, q)
            for r in range(2):
                if cfg["run"][r]:
                    rm, rv, brm, brv = c["run"][(r, cfg["cbias"][r])]
                    _close(f"{tag} running_mean{r} bias={cfg['cbias'][r]}", _np(out[f"rmean{r}"]), _np(rm), _np(brm))
                    _close(f"{tag} running_var{r}", _np(out[f"rvar{r}"]), _np(rv), _np(brv))
                if cfg["nbt"][r]:
                    assert int(out[f"nbt{r}"]) == NBT0 + 1
        g = _fold_bwd(dev, first, Co, TV, n_pos)
        for q in ("dX", "dgamma", "dbeta", "dGc"):
            _close(f"{tag} {q}", _np(g[q]), ref[q], bound[q])
        print(f"NOTE {tag} dGc error / double-only bound {float(np.max(np.abs(_np(g['dGc']) - ref['dGc']) / np.maximum(c['dGc_u64'], 1e-300))):.1f}")
        g2 = _fold_bwd(dev, first, Co, TV, n_pos)
        for q in ("dX", "dgamma", "dbeta", "dGc"):
            assert _same_bits(g2[q], g[q]), ("backward repeat", q)


def test_lowrank_fold_refusals():
    """T V = 513 (COSKAD_ERR_SHAPE from both entry points, nothing written), latent != 8 through coskad_lowrank_fold_ok, and running
    buffers given on one side only (COSKAD_ERR_ARG)"""
    lib = _lib().lib()
    st = _stream()
    assert lib.coskad_lowrank_fold_ok(8, 512) == 1 and lib.coskad_lowrank_fold_ok(8, 513) == 0 and lib.coskad_lowrank_fold_ok(8, 0) == 0
    assert lib.coskad_lowrank_fold_ok(16, 204) == 0 and lib.coskad_lowrank_fold_ok(7, 204) == 0 and lib.coskad_lowrank_fold_ok(9, 204) == 0
    Co = 2
    for TV, one_sided, rc in ((513, False, ERR_SHAPE), (20, True, ERR_ARG)):
        d = R.fold_inputs(Co, TV, 3, seed=5)
        dev = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
        o = {"Mw": _out((Co * TV, K9 - 1), NAN), "Mb": _out((Co * TV,), NAN), "saved": _out((3, 2, Co), NAN, torch.float64),
             "xbar": _out((2, K9, Co), NAN, torch.float64), "xx": _out((2, Co, K9, K9), NAN, torch.float64), "dX": _out((2, K9, Co, TV), NAN),
             "dgamma": _out((2, Co), NAN), "dbeta": _out((Co,), NAN), "dGc": _out((Co, K9, K9), NAN, torch.float64)}
        p = {k: v[1].data_ptr() for k, v in o.items()}
        q = {k: v.data_ptr() for k, v in dev.items()}
        rm0, rv0 = dev["rmean0"].clone(), dev["rvar0"].clone()
        got = lib.coskad_lowrank_fold_fwd_f32(q["X"], q["G"], q["gamma0"], q["beta0"], None, q["rmean0"], None if one_sided else q["rvar0"], None,
                                              0.1, 1e-5, q["gamma1"], q["beta1"], None, None, None, None, 0.1, 1e-5, d["n_pos"], p["Mw"], p["Mb"],
                                              p["saved"], p["xbar"], p["xx"], Co, TV, st)
        assert got == rc, (TV, one_sided, got)
        if not one_sided:
            z64 = torch.zeros(3 * 2 * Co + 2 * K9 * Co + 2 * Co * K9 * K9, dtype=torch.float64, device="cuda")
            got = lib.coskad_lowrank_fold_bwd_f32(q["X"], q["G"], q["dMw"], q["dMb"], z64.data_ptr(), z64.data_ptr(), z64.data_ptr(), q["gamma0"],
                                                  q["gamma1"], d["n_pos"], p["dX"], p["dgamma"], p["dbeta"], p["dGc"], Co, TV, st)
            assert got == rc, ("bwd", TV, got)
        torch.cuda.synchronize()
        _intact(o, "fold refusal")
        assert all(_all_nan(v) for _, v in o.values())
        assert _same_bits(dev["rmean0"], rm0) and _same_bits(dev["rvar0"], rv0)


# ======================================================================================================================================
# C. mlp_head, both kernel sets
# ======================================================================================================================================

MLP_FAST = [(2, 1, 1), (63, 16, 16), (64, 16, 16), (65, 7, 12), (130, 12, 7), (513, 16, 1), (1024, 8, 8), (4099, 16, 16)]
MLP_GENERAL = [(5, 17, 3), (77, 24, 16), (256, 33, 17), (257, 8, 40), (300, 64, 64)]
MLP_EVAL_ONLY = [(1, 16, 16)]                       # B = 1: eval mode only (a batch of one has no batch statistics to train on)
MLP_EPS, MLP_MOM = 1e-5, 0.1
KINK_CAP = 1e-3


@functools.lru_cache(maxsize=None)
def mlp_case(B, H, L, training):
    """Inputs, the double reference (kernel_refs.mlp_head with autograd) and every bound of one mlp_head case.  No device.

    Statistics (train; both kernel sets sum in double: k_stats two-pass, k_stats16 as sum y^2 - m sum y): the float32 `stat` is one
    conversion of a double value,
      e_mean = U32 |mean| + (B + 8) U64 mean|y|,   dvar = 2 (B + 8) U64 (mean(y^2) + mean^2)  (the cancellation of the one-pass form),
      e_inv = U32 inv + inv / (2 (var + eps)) dvar + 4 U64 inv;  eval: the mean is the buffer itself, inv = 1.f / sqrtf(rvar + eps): 5 U32 inv.
      running mean / variance: (1 - mom) old + mom new in double, one conversion: (U32 + 8 U64) M + mom (the double terms above).
    Forward: sc = gamma inv (1), sf = beta - sc mean (2), y2 = fmaf(y, sc, sf) (1): the mean's term passes 4 roundings:
      e_y2f = 4 U32 M_y2 + |gamma| inv e_mean + |gamma| |y - mean| e_inv,   M_y2 = |gamma| inv (|y| + |mean|) + |beta|
      z = b2 + H fmaf of relu(y2), relu 1-Lipschitz:  e_z = e_y2f |W2|^T + H U32 (relu(y2) |W2|^T + |b2|)    -- nothing is left out
    Backward: xh = (y - mean) inv (2), y2 = fmaf(gamma, xh, beta) (1):
      e_xh = 2 U32 |xh| + inv e_mean + |y - mean| e_inv,   e_y2b = |gamma| e_xh + U32 |y2|
      kink: y2 != 0 and |y2| <= max(e_y2f, e_y2b) -- the forward and the backward evaluate the gate from different float32
      expressions, and either may sit on the other side of 0 from the double y2 there.  These elements are left out of dy and widen
      their feature's sums by what they could add (their da, resp. da xh); an exact 0 (gamma = beta = 0) is closed on both sides.
      da = L fmaf from 0.f: e_da = L U32 M_da, M_da = |dz| |W2|
      red0 = sum_n dy2 (= dbeta), red1 = sum_n dy2 xh (= dgamma): general set in double over B clips, one conversion: k = L + 1 (red1: the
      double product of two float32 is exact); fast set: dy2 xh in float32 (1), 64 rows of a block added in turn (rows - 1), the blocks
      in double, one conversion: k = L + rows (red0), L + 1 + rows (red1).  red1 also carries sum gate M_da e_xh.  `accumulate`: + 1.
      dW2 = sum_n dz relu(y2): relu 1-Lipschitz, so no widening: sum |dz| e_y2b + (fast: one fmaf per row of the block, `rows`) + one
      conversion (+ 1);  db2: general (1 + acc) U32, B in double; fast (rows - 1 + 1 + acc), blocks in double
      dy1 = (inv gamma) (dy2 - red0 invB - xh red1 invB): invB (1), four multiplies / subtractions on the longest term (4), inv gamma
      (1), the product (1): 6 U32 |gamma| inv M_r + |gamma| inv (gate e_da + e_red0 / B + |xh| e_red1 / B + e_xh |red1| / B) + |gamma| M_r e_inv,
      M_r = gate M_da + M_red0 / B + |xh| M_red1 / B;  eval: (inv gamma) dy2: 2 U32 + the da and inv terms."""
    d = R.mlp_inputs(B, H, L, seed=100 * B + 10 * H + L)
    fast = R.mlp_fast(H, L)
    leaf = lambda t: dd(t).clone().requires_grad_(True)
    y, gam, bet, W2, b2 = (leaf(d[k]) for k in ("y", "gamma", "beta", "W2", "b2"))
    rm0, rv0 = dd(d["rmean"]), dd(d["rvar"])
    f = R.mlp_head(y, gam, bet, W2, b2, MLP_EPS, training, rm0, rv0)
    dz = dd(d["dz"])
    gy, gg, gb, gW, gb2 = torch.autograd.grad(f["z"], [y, gam, bet, W2, b2], dz)
    f = {k: v.detach() for k, v in f.items()}
    y, gam, bet, W2, b2 = (t.detach() for t in (y, gam, bet, W2, b2))
    mean, var, inv, xh, y2 = f["mean"], f["var"], f["inv"], f["xh"], f["y2"]
    eps = R.f32(MLP_EPS)
    ref = dict(z=f["z"], z_nobias=f["z"] - b2, mean=mean, inv=inv, dy=gy, dgamma=gg, dbeta=gb, dW2=gW, db2=gb2)
    bound = {}
    if training:
        dbl = (B + 8) * U64
        absy, sq = y.abs().mean(0), (y * y).mean(0)
        dvar = 2 * dbl * (sq + mean * mean)
        e_mean = U32 * mean.abs() + dbl * absy
        e_inv = U32 * inv + 0.5 * inv / (var + eps) * dvar + 4 * U64 * inv
        mom = R.f32(MLP_MOM)
        unbf = B / (B - 1.0) if B > 1 else 1.0
        ref["rm"], ref["rv"] = (1 - mom) * rm0 + mom * mean, (1 - mom) * rv0 + mom * var * unbf
        bound["rm"] = (U32 + 8 * U64) * ((1 - mom) * rm0.abs() + mom * mean.abs()) + mom * dbl * absy
        bound["rv"] = (U32 + 8 * U64) * ((1 - mom) * rv0.abs() + mom * var * unbf) + mom * unbf * dvar
    else:
        e_mean, e_inv = torch.zeros_like(mean), 5 * U32 * inv
    bound["mean"], bound["inv"] = e_mean, e_inv
    ag = gam.abs()
    dev_ = (y - mean).abs()
    My2 = ag * inv * (y.abs() + mean.abs()) + bet.abs()
    e_y2f = 4 * U32 * My2 + ag * inv * e_mean + ag * dev_ * e_inv
    a = torch.relu(y2)
    bound["z"] = e_y2f @ W2.abs().T + H * U32 * (a @ W2.abs().T + b2.abs())
    bound["z_nobias"] = e_y2f @ W2.abs().T + H * U32 * (a @ W2.abs().T)
    e_xh = 2 * U32 * xh.abs() + inv * e_mean + dev_ * e_inv
    e_y2b = ag * e_xh + U32 * y2.abs()
    kink = (y2 != 0) & (y2.abs() <= torch.maximum(e_y2f, e_y2b))
    gate = (y2 > 0).double()
    Mda = dz.abs() @ W2.abs()
    da = dz @ W2
    e_da = L * U32 * Mda
    kM = kink.double() * Mda * (1 + L * U32)
    rows = min(B, R.MLP_RB)
    nblk = ceil_div(B, R.MLP_RB)
    cnt = (nblk if fast else B) + 8
    MB, MG = (gate * Mda).sum(0), (gate * Mda * xh.abs()).sum(0)
    red0, red1 = (gate * da).sum(0), (gate * da * xh).sum(0)
    k0, k1 = (L + rows, L + 1 + rows) if fast else (L + 1, L + 1)
    e_red0 = (k0 * U32 + cnt * U64) * MB + kM.sum(0)
    e_red1 = (k1 * U32 + cnt * U64) * MG + (gate * Mda * e_xh).sum(0) + (kM * (xh.abs() + e_xh)).sum(0)
    MW = dz.abs().T @ a
    e_W = dz.abs().T @ e_y2b + cnt * U64 * MW
    kW = rows + 1 if fast else 1
    Mb2 = dz.abs().sum(0)
    kb2 = rows if fast else 1
    for acc in (False, True):
        pr, s = (PRIOR if acc else 0.0), ("+" if acc else "")
        bound["dbeta" + s] = e_red0 + int(acc) * U32 * (MB + pr)
        bound["dgamma" + s] = e_red1 + int(acc) * U32 * (MG + pr)
        bound["dW2" + s] = e_W + (kW + int(acc)) * U32 * (MW + pr)
        bound["db2" + s] = ((kb2 + int(acc)) * U32 + cnt * U64) * (Mb2 + pr)
    if training:
        Mr = gate * Mda + MB / B + xh.abs() * MG / B
        e_r = gate * e_da + e_red0 / B + xh.abs() * e_red1 / B + e_xh * red1.abs() / B
        bound["dy"] = 6 * U32 * ag * inv * Mr + ag * inv * e_r + ag * Mr * e_inv
    else:
        bound["dy"] = ag * inv * gate * (2 * U32 * Mda + e_da) + ag * gate * Mda * e_inv
    return dict(d=d, ref={k: _np(v) for k, v in ref.items()}, bound={k: _np(v) for k, v in bound.items()}, kink=_np(kink),
                share=float(kink.double().mean()))


def _mlp_fwd(dev, B, H, L, training, bias=True, running=True):
    lib = _lib()
    n = lib.lib().coskad_mlp_head_ws_floats(B, H, L)
    bufs = {"z": _out((B, L), NAN), "stat": _out((n,), NAN), "rm": _out((H,), 0.0), "rv": _out((H,), 0.0)}
    bufs["rm"][1].copy_(dev["rmean"]); bufs["rv"][1].copy_(dev["rvar"])
    nbt = torch.full((), NBT0, dtype=torch.int64, device="cuda")
    lib.call("coskad_mlp_head_fwd_f32", dev["y"], dev["gamma"], dev["beta"], bufs["rm"][1] if running else None, bufs["rv"][1] if running else None,
             nbt if running else None, MLP_MOM, MLP_EPS, 1 if training else 0, dev["W2"], dev["b2"] if bias else None, bufs["z"][1],
             bufs["stat"][1], B, H, L, _stream())
    _intact(bufs, "mlp fwd")
    out = {k: v[1] for k, v in bufs.items()}
    out["nbt"] = nbt
    return out


def _mlp_bwd(dev, stat, B, H, L, training, acc=False, with_db2=True):
    lib = _lib()
    fill = PRIOR if acc else NAN
    n = lib.lib().coskad_mlp_head_ws_floats(B, H, L)
    bufs = {"dy": _out((B, H), NAN), "dgamma": _out((H,), fill), "dbeta": _out((H,), fill), "dW2": _out((L, H), fill), "db2": _out((L,), fill),
            "red": _out((n,), NAN)}
    lib.call("coskad_mlp_head_bwd_f32", dev["y"], stat, dev["gamma"], dev["beta"], dev["W2"], dev["dz"], bufs["dy"][1], bufs["dgamma"][1],
             bufs["dbeta"][1], bufs["dW2"][1], bufs["db2"][1] if with_db2 else None, bufs["red"][1], 1 if training else 0, 1 if acc else 0,
             B, H, L, _stream())
    _intact(bufs, "mlp bwd")
    return {k: v[1] for k, v in bufs.items()}


def _mlp_run(B, H, L, training):
    c = mlp_case(B, H, L, training)
    d, ref, bound = c["d"], c["ref"], c["bound"]
    assert c["share"] <= KINK_CAP, c["share"]
    dev = {k: v.cuda() for k, v in d.items()}
    tag = f"mlp {B}x{H}x{L} {'train' if training else 'eval'}"
    f = _mlp_fwd(dev, B, H, L, training)
    _close(f"{tag} z", _np(f["z"]), ref["z"], bound["z"])
    _close(f"{tag} stat.mean", _np(f["stat"][:H]), ref["mean"], bound["mean"])
    _close(f"{tag} stat.invstd", _np(f["stat"][H:2 * H]), ref["inv"], bound["inv"])
    if training:
        _close(f"{tag} running_mean", _np(f["rm"]), ref["rm"], bound["rm"])
        _close(f"{tag} running_var", _np(f["rv"]), ref["rv"], bound["rv"])
        assert int(f["nbt"]) == NBT0 + 1
        bare = _mlp_fwd(dev, B, H, L, True, running=False)         # no running buffers, no counter
        assert _same_bits(bare["z"], f["z"]) and _same_bits(bare["stat"][:2 * H], f["stat"][:2 * H])
        assert _same_bits(bare["rm"], dev["rmean"]) and _same_bits(bare["rv"], dev["rvar"])
    else:
        assert _same_bits(f["rm"], dev["rmean"]) and _same_bits(f["rv"], dev["rvar"]) and int(f["nbt"]) == NBT0
        assert _same_bits(f["stat"][:H], dev["rmean"])
    again = _mlp_fwd(dev, B, H, L, training)
    for q in ("z", "rm", "rv"):
        assert _same_bits(again[q], f[q]), ("repeat", q)
    assert _same_bits(again["stat"][:2 * H], f["stat"][:2 * H])
    nob = _mlp_fwd(dev, B, H, L, training, bias=False)
    _close(f"{tag} z without b2", _np(nob["z"]), ref["z_nobias"], bound["z_nobias"])
    if training and H >= R.MLP_PLANTS:                             # the constant column: a variance of exactly 0 on both sides
        assert float(ref["inv"][3]) == pytest.approx(1 / np.sqrt(R.f32(MLP_EPS)), rel=1e-12)
    # backward, from the kernel's own stat
    g = _mlp_bwd(dev, f["stat"], B, H, L, training)
    keep = ~c["kink"]
    _close(f"{tag} dy", _np(g["dy"]), ref["dy"], bound["dy"], where=keep)
    for q in ("dgamma", "dbeta", "dW2", "db2"):
        _close(f"{tag} {q}", _np(g[q]), ref[q], bound[q])
    if H >= R.MLP_PLANTS:
        gn = _np(g["dy"])
        assert not gn[:, 1].any() and not gn[:, 2].any(), "dy of a feature with gamma = 0"
        assert float(g["dgamma"][1]) == 0.0 and float(g["dbeta"][1]) == 0.0, "the closed gate (gamma = beta = 0)"
        assert float(ref["dgamma"][2]) != 0.0
    g2 = _mlp_bwd(dev, f["stat"], B, H, L, training)
    for q in ("dy", "dgamma", "dbeta", "dW2", "db2"):
        assert _same_bits(g2[q], g[q]), ("backward repeat", q)
    nodb = _mlp_bwd(dev, f["stat"], B, H, L, training, with_db2=False)
    for q in ("dy", "dgamma", "dbeta", "dW2"):
        assert _same_bits(nodb[q], g[q]), ("without db2", q)
    assert _all_nan(nodb["db2"]), "db2 written though absent"
    ga = _mlp_bwd(dev, f["stat"], B, H, L, training, acc=True)
    assert _same_bits(ga["dy"], g["dy"])
    for q in ("dgamma", "dbeta", "dW2", "db2"):
        _close(f"{tag} {q} accumulate", _np(ga[q]), ref[q] + PRIOR, bound[q + "+"])


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,H,L", MLP_FAST)
def test_mlp_head_fast_path(B, H, L, training):
    """hidden, out <= 16 (k_stats16, k_apply16, k_bwd_reduce16, k_bwd_apply16): 1, 2, 3, 9, 16 and 65 blocks of 64 rows -- sum_parts'
    unroll of eight with remainders 1, 2, 3, 1, 0 and 1 -- ragged last blocks, L > H and H > L.  Bounds and modes: mlp_case, _mlp_run."""
    assert R.mlp_fast(H, L)
    _mlp_run(B, H, L, training)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,H,L", MLP_GENERAL)
def test_mlp_head_general_path(B, H, L, training):
    """one block per feature (k_stats, k_apply, k_bwd_reduce, k_bwd_apply): H or L above 16 up to 64, fewer clips than a block's
    threads, one more than them, H <= 16 with L > 16"""
    assert not R.mlp_fast(H, L)
    _mlp_run(B, H, L, training)


@pytest.mark.parametrize("B,H,L", MLP_EVAL_ONLY)
def test_mlp_head_single_clip_eval(B, H, L):
    """one clip through the fast set's one ragged block, eval mode (the running statistics normalise; nothing is summed over a batch)"""
    _mlp_run(B, H, L, False)
