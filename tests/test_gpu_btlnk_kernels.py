"""Kernel-level checks of the bottleneck projection z = W . PReLU(U) + b and its backward: csrc/bottleneck.hip (L <= 16: the direct
forward coskad_btlnk_fwd_f32, the split-K forward coskad_btlnk_fwd_ws_f32 / coskad_btlnk_fwd_parts_f32, coskad_btlnk_bwd_f32),
csrc/btlnk_chain.hip (coskad_btlnk_bwd_chain_f32, and coskad_btlnk_bwd_chain_head_f32 against the launches it replaces) and
csrc/btlnk_wide.hip (16 < L <= 512), called directly with guard bands around every output, against kernel_refs.btlnk /
kernel_refs.top_layer_sums in double with autograd's gradients.

Every bound is  k * U32 * M  (+ (count + 8) * U64 * M for what the kernels sum in double): M the double sum of the absolute values
of the element's terms, k the float32 roundings on the longest chain a term passes through, read from the kernel -- the functions
k_* below, each with its derivation; the chain lengths come from the plan restatements of kernel_refs.py, which
test_kernel_refs_host.py holds against the library's own size queries.  An f32 MFMA counts one rounding per product (it is an fmaf
chain); a product with an operand the kernel zero-fills is exact and not counted.  The library is built with -ffp-contract=off, so
every add and multiply written in a kernel rounds once.  Nothing is left out of a comparison: the PReLU gate is the sign of the float32
input itself, which both sides read exactly.  Inputs: kernel_refs.btlnk_inputs (magnitudes 1e-3 / 1 / 30 mixed per element, exact
+0.0 / -0.0 planted where a tile ends).  Each check prints `RATIO <name> <largest error / bound>` (DESIGN.md 6.1 records a run)."""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_refs import U32, U64, ceil_div, dd
from test_gpu_head_rides import _same_bits
from test_gpu_wide_kernels import _close
from test_gpu_wide_latent import SENT, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

HID = 64
SLOPES = [None, 0.25, 0.0, -0.5, 1.0]
PRIOR = 0.5                       # what `accumulate` adds onto
KEEP = 7.0                        # a dslope buffer the call must not touch

# ---- the shapes and the edge each is listed for (asserted by test_kernel_refs_host.py from the plan restatements) -----------------

FWD_LS = (1, 5, 15, 16)
FWD_BS = (1, 15, 16, 17, 63, 64, 65, 130)
FWD_K_DIRECT = (4, 20, 48, 272, 820)        # a K % 16 tail; 1, 2, 3, 17 and 52 k-steps over eight waves
FWD_K_SPLIT = (16, 80, 272, 1296)           # 1, 5, 17 and 81 k-steps over 16 wave groups: empty and odd-length slices
FWD_SUBSETS = (1, 7, 64)

BWD_SHAPES = [(1, 4, 1), (15, 20, 5), (17, 260, 16), (100, 272, 15), (330, 13056, 16), (1041, 272, 16), (1041, 1280, 5), (145, 272, 8)]

CHAIN_SHAPES = [(1, 4, 16, 1), (17, 20, 32, 8), (37, 136, 16, 16), (40, 204, 32, 16), (100, 600, 32, 16), (700, 204, 32, 9),
                (1120, 20, 16, 16), (33, 272, 32, 5)]
CHAIN_SLOPES = [None, 0.25, 0.0]
IN_SLOPES = [None, 0.2]

RIDE_SHAPES = [(17, 20, 32, 8), (100, 600, 32, 16), (600, 20, 16, 16)]

# the last one is not in the issue's table: none of its shapes has a dW clip chunk longer than 16 (every B <= 1024 gives
# ceil(B / 64) <= 16), so B = 1040 was added for that edge
WIDE_SHAPES = [(1, 3, 17), (127, 100, 32), (129, 272, 33), (300, 272, 64), (129, 1030, 65), (40, 129, 129), (20, 272, 512),
               (260, 100, 200), (1040, 36, 40)]


# ---- k: float32 roundings on the longest chain ---------------------------------------------------------------------------------------

def k_fwd_direct(K, pre, bias):
    """k_btlnk_fwd: a wave owns `per` = ceil(ceil(K / 16) / 8) k-steps of 16 products (one MFMA accumulator: at most min(K, 16 per)
    products that are not zero-filled), the eight wave partials are added in turn to 0.f (the first add is exact: 7), then the bias
    (1); PReLU's a u on the operand (1)."""
    per = ceil_div(ceil_div(K, 16), 8)
    return min(K, 16 * per) + 7 + int(bias) + int(pre)


def k_fwd_split(K, KS, pre, bias):
    """k_btlnk_fwd_t + k_btlnk_fwd_sum: wave group g of 4 KS owns the k-steps [nsteps g / G, nsteps (g + 1) / G) (16 products each), the
    four waves of a block are added as (r0 + r1) + (r2 + r3) (2), the KS slices in turn to 0.f (KS - 1), the bias (1), a u (1)."""
    nsteps, G = K // 16, 4 * KS
    longest = max(nsteps * (g + 1) // G - nsteps * g // G for g in range(G))
    return 16 * longest + 2 + (KS - 1) + int(bias) + int(pre)


def k_du(L, pre):
    """dU = (sum_j dz W) gate: one MFMA chain over the L latents (all three files), then a g on the slope's side (1)"""
    return L + int(pre)


def k_dw(chunk, pre, acc):
    """dW: one MFMA chain over the clips of a chunk (`chunk` products, the operand PReLU(u) carries a u: 1), the chunks' slabs summed
    in double, the conversion to float32 (1) and out + . under `accumulate` (1)"""
    return chunk + int(pre) + 1 + int(acc)


def k_db(acc):
    """db: dz summed in double, the conversion (1), the accumulate (1)"""
    return 1 + int(acc)


def k_da_narrow(L, chunk, acc):
    """k_btlnk_bwd's slope gradient: g (L products) times u (1), four of them added as (t0 + t1) + (t2 + t3) (2), added to the lane's
    sum once per clip the lane group owns (chunk / 4), wave_sum (6), the four waves (2); the blocks' partials summed in double, the
    conversion (1), the accumulate (1)"""
    return L + 1 + 2 + chunk // 4 + 6 + 2 + 1 + int(acc)


def k_da_chain(L, chunk, acc):
    """k_btlnk_bwd_stats: g (L) times u (1), added to the lane's sum one by one, 8 channels x 4 clip registers per 16-clip tile
    (2 chunk), wave_sum (6), the eight waves as a tree (3), conversion (1), accumulate (1)"""
    return L + 1 + 2 * chunk + 6 + 3 + 1 + int(acc)


def k_da_wide(L, acc):
    """k_wide<DX>: g (L) times u (1), the lane's 4 x 4 x 4 = 64 accumulator elements added one by one (64), wave_sum (6), four waves
    (2), conversion (1), accumulate (1)"""
    return L + 1 + 64 + 6 + 2 + 1 + int(acc)


def k_fwd_wide(K, L, pre, bias):
    """k_wide<FWD> + k_wfwd_sum: one MFMA chain over a slice of K (at most min(rchunk, K) products), the slices in turn to 0.f
    (KS - 1), the bias (1), a u (1)"""
    return min(R.wide_fwd_rchunk(K, L), K) + (R.wide_fwd_slices(K, L) - 1) + int(bias) + int(pre)


def k_chain_pq(chunk, xact):
    """P / Q of one partial row: a wave's accumulator takes 8 positions x the chunk's clips (8 chunk products of the stored float32
    dU tile, which the reference reads back, with the float32 Z / input), the two position halves are added once (1); Q's operand
    PReLU(x) carries a_in x (1).  The rows are summed in double."""
    return 8 * chunk + 1 + int(xact)


def k_chain_s(chunk):
    """s of one partial row: the lane adds its 8 positions x 4 clip registers per tile one by one (2 chunk), two butterfly adds over
    the lane groups (2), the position halves (1)"""
    return 2 * chunk + 2 + 1


def _bd(k, M, count=None):
    return (k * U32 + (0.0 if count is None else (count + 8) * U64)) * M


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------

def _lib():
    from coskad_amd import _lib as L
    return L


def _stream():
    from coskad_amd import ops
    return ops._stream()


def _slope_dev(a):
    return None if a is None else torch.tensor([a], dtype=torch.float32).cuda()


def _slope_ref(a):
    return None if a is None else R.f32(a)


def _out(shape, fill):
    """a guarded output (SENT on both sides) holding `fill` -> (parent, view)"""
    n = int(np.prod(shape))
    buf, v = _guarded(n)
    v.fill_(fill)
    return buf, v.view(*shape)


def _scratch(nbytes):
    """a workspace of all-ones bytes: a partial the kernels do not write is a NaN in whatever sums it"""
    return torch.full((int(nbytes) + 4,), 0xFF, dtype=torch.uint8, device="cuda")


_bits = _same_bits               # bitwise equality, NaN patterns included


def _np(t):
    return t.detach().cpu().numpy()


# ---- (a) narrow forward --------------------------------------------------------------------------------------------------------------

BMAX = max(FWD_BS)


def _fwd_ref(d, a, bias):
    """double z [BMAX, L] and M = sum |W| |PReLU(U)| + |b|; rows do not depend on the batch they sit in"""
    U, W = dd(d["U"]), dd(d["W"])
    b = dd(d["b"]) if bias else None
    z = R.btlnk(U, _slope_ref(a), W, b)
    X = U if a is None else R.prelu(U, _slope_ref(a))
    M = X.abs() @ W.abs().T + (b.abs() if bias else 0.0)
    return _np(z), _np(M)


def _call_fwd_direct(dev, s, bias, B, K, L):
    buf, z = _out((B, L), float("nan"))
    _lib().call("coskad_btlnk_fwd_f32", dev["U"], dev["W"], dev["b"] if bias else None, s, z, B, K, L, _stream())
    _guards_intact(buf, "fwd_f32 z")
    return z


def _call_fwd_ws(dev, s, bias, B, K, L):
    lib = _lib()
    nbytes = lib.lib().coskad_btlnk_fwd_ws_bytes_l(B, K, L)
    ws = _scratch(nbytes)
    buf, z = _out((B, L), float("nan"))
    lib.call("coskad_btlnk_fwd_ws_f32", dev["U"], dev["W"], dev["b"] if bias else None, s, z, ws, nbytes, B, K, L, _stream())
    _guards_intact(buf, "fwd_ws z")
    return z


def _call_fwd_parts(dev, s, B, K, L, KS):
    buf, part = _out((KS, B, 16), float("nan"))
    _lib().call("coskad_btlnk_fwd_parts_f32", dev["U"], dev["W"], s, part, part.numel() * 4, B, K, L, _stream())
    _guards_intact(buf, "fwd_parts part")
    return part


@pytest.mark.parametrize("L", FWD_LS)
@pytest.mark.parametrize("K", FWD_K_DIRECT)
def test_narrow_forward_direct(K, L):
    """coskad_btlnk_fwd_f32 (k_btlnk_fwd; since ops.btlnk_fwd always takes the split-K path when K % 16 == 0, this file is the only
    caller of the kernel) at every B of FWD_BS, every slope, with and without a bias: z within k_fwd_direct U32 M of the double
    reference, a repeat call bit-equal."""
    d = R.btlnk_inputs(BMAX, K, L, seed=7 * K + L)
    dev = {k: v.cuda() for k, v in d.items()}
    got, ref, bound = [], [], []
    for a in SLOPES:
        s = _slope_dev(a)
        for bias in (True, False):
            zr, M = _fwd_ref(d, a, bias)
            k = k_fwd_direct(K, a is not None, bias)
            for B in FWD_BS:
                z = _call_fwd_direct(dev, s, bias, B, K, L)
                got.append(_np(z).ravel()); ref.append(zr[:B].ravel()); bound.append(k * U32 * M[:B].ravel())
            assert _bits(_call_fwd_direct(dev, s, bias, BMAX, K, L), z), ("repeat", a, bias)
    _close(f"fwd_f32 K={K} L={L} z", np.concatenate(got), np.concatenate(ref), np.concatenate(bound))


@pytest.mark.parametrize("L", FWD_LS)
@pytest.mark.parametrize("K", FWD_K_SPLIT)
def test_narrow_forward_split_k(K, L):
    """coskad_btlnk_fwd_ws_f32 and coskad_btlnk_fwd_parts_f32 (k_btlnk_fwd_t, k_btlnk_fwd_sum) on the same inputs: z within
    k_fwd_split U32 M; z of every smaller batch -- FWD_BS and FWD_SUBSETS -- bit-equal to the leading rows of the largest (the
    bit-exact chunking ops.py relies on); the float32 prefix sum of the partials in slice order plus the bias (0.f without one, as
    k_btlnk_fwd_sum writes it) bit-equal to z for whatever coskad_btlnk_fwd_ks() is, columns L..15 of `part` not looked at; a repeat
    call bit-equal; and the direct kernel on the same inputs within the sum of the two bounds."""
    KS = _lib().lib().coskad_btlnk_fwd_ks()
    d = R.btlnk_inputs(BMAX, K, L, seed=11 * K + L)
    dev = {k: v.cuda() for k, v in d.items()}
    got, ref, bound, gap, gapb = [], [], [], [], []
    for a in SLOPES:
        s = _slope_dev(a)
        for bias in (True, False):
            zr, M = _fwd_ref(d, a, bias)
            k = k_fwd_split(K, KS, a is not None, bias)
            zfull = _call_fwd_ws(dev, s, bias, BMAX, K, L)
            assert _bits(_call_fwd_ws(dev, s, bias, BMAX, K, L), zfull), ("repeat", a, bias)
            for B in sorted(set(FWD_BS + FWD_SUBSETS)):
                z = _call_fwd_ws(dev, s, bias, B, K, L)
                assert _bits(z, zfull[:B]), ("batch independence", a, bias, B)
                part = _np(_call_fwd_parts(dev, s, B, K, L, KS))
                acc = np.zeros((B, L), np.float32)
                for i in range(KS):
                    acc = acc + part[i, :, :L]
                acc = acc + (d["b"].numpy() if bias else np.float32(0.0))
                assert acc.dtype == np.float32 and np.array_equal(acc.view(np.int32), _np(z).view(np.int32)), ("parts", a, bias, B)
                got.append(_np(z).ravel()); ref.append(zr[:B].ravel()); bound.append(k * U32 * M[:B].ravel())
            zd = _call_fwd_direct(dev, s, bias, BMAX, K, L)
            gap.append((_np(zd).astype(np.float64) - _np(zfull)).ravel())
            gapb.append((k + k_fwd_direct(K, a is not None, bias)) * U32 * M.ravel())
    _close(f"fwd_ws K={K} L={L} z", np.concatenate(got), np.concatenate(ref), np.concatenate(bound))
    gap = np.concatenate(gap)
    _close(f"fwd_ws K={K} L={L} direct - split", gap, np.zeros_like(gap), np.concatenate(gapb))


# ---- the backward's reference and checks (narrow, chain and wide alike) ---------------------------------------------------------------

def _bwd_ref(d, a):
    """float64 autograd of sum(dz * btlnk(U, a, W, b)) and the M of every quantity"""
    U, W, b, dz = (dd(d[k]) for k in ("U", "W", "b", "dz"))
    leaves = [U.requires_grad_(True), W.requires_grad_(True), b.requires_grad_(True)]
    s = None
    if a is not None:
        s = torch.tensor(R.f32(a), dtype=torch.float64, requires_grad=True)
        leaves.append(s)
    g = torch.autograd.grad(R.btlnk(U, s, W, b), leaves, dz)
    U, W = U.detach(), W.detach()
    G = dz.abs() @ W.abs()                                           # sum_j |dz W| per element of U
    gate = torch.ones_like(U) if a is None else torch.where(U > 0, torch.ones_like(U), torch.full_like(U, abs(R.f32(a))))
    X = U if a is None else R.prelu(U, R.f32(a))
    ref = dict(dU=g[0], dW=g[1], db=g[2])
    M = dict(dU=G * gate, dW=dz.abs().T @ X.abs(), db=dz.abs().sum(0))
    if a is not None:
        ref["dslope"] = g[3].reshape(1)
        M["dslope"] = (G * U.abs() * (U < 0)).sum().reshape(1)
    return {k: _np(v) for k, v in ref.items()}, {k: _np(v) for k, v in M.items()}


def _call_bwd(dev, s, B, K, L, accumulate, absent=(), keep_slope=False):
    """coskad_btlnk_bwd_f32 onto NaN (overwrite) or PRIOR (accumulate); dslope holds KEEP when the call must not write it"""
    lib = _lib()
    fill = PRIOR if accumulate else float("nan")
    bufs = {"dU": _out((B, K), float("nan")), "dW": _out((L, K), fill), "db": _out((L,), fill),
            "dslope": _out((1,), KEEP if keep_slope else fill)}
    arg = {k: (None if k in absent else v[1]) for k, v in bufs.items()}
    nbytes = lib.lib().coskad_btlnk_bwd_ws_bytes(B, K, L)
    ws = _scratch(nbytes)
    lib.call("coskad_btlnk_bwd_f32", dev["U"], dev["W"], dev["dz"], s, arg["dU"], arg["dW"], arg["db"], arg["dslope"], ws, nbytes,
             1 if accumulate else 0, B, K, L, _stream())
    for k, (buf, _) in bufs.items():
        _guards_intact(buf, "bwd " + k)
    return {k: v[1] for k, v in bufs.items()}


def _check_grads(tag, out, ref, M, ks, counts, accumulate, skip=()):
    """dU / dW / db / dslope of one call against the reference; ks: {quantity: k}, counts: {quantity: terms summed in double};
    -> the bounds, for comparisons between two kernels"""
    bounds = {}
    for q in ("dU", "dW", "db", "dslope"):
        if q not in ref or q in skip:
            continue
        prior = PRIOR if accumulate and q != "dU" else 0.0
        bounds[q] = _bd(ks[q], M[q] + prior, counts.get(q))
        _close(f"{tag} {q}", _np(out[q]), ref[q] + prior, bounds[q])
    return bounds


def _bwd_modes(tag, call, ref, M, ks_of, counts, pre):
    """the modes every backward entry point is put through: overwrite onto NaN and accumulate onto PRIOR within bounds, a repeat
    call bit-equal, db and dslope absent in turn with the other outputs bit-equal, and -- without a slope -- a dslope buffer that is
    given left untouched.  call(accumulate, absent, keep_slope) -> outputs; -> (the overwrite call's outputs, its bounds)"""
    full = call(False, (), not pre)
    bounds = _check_grads(tag, full, ref, M, ks_of(False), counts, False)
    if not pre:
        assert _bits(full["dslope"], torch.full((1,), KEEP, device="cuda")), "dslope written without a slope"
    grads = ("dU", "dW", "db", "dslope")
    again = call(False, (), not pre)
    for q in grads:
        assert _bits(again[q], full[q]), (tag, "repeat", q)
    accd = call(True, (), not pre)
    _check_grads(tag + " accumulate", accd, ref, M, ks_of(True), counts, True, skip=("dU",))
    assert _bits(accd["dU"], full["dU"])                             # dU is never accumulated: held to the reference above
    if not pre:
        assert _bits(accd["dslope"], torch.full((1,), KEEP, device="cuda")), "dslope accumulated without a slope"
    for gone in ("db", "dslope"):
        part = call(False, (gone,), not pre)
        for q in grads:
            if q != gone:
                assert _bits(part[q], full[q]), (tag, "without " + gone, q)
    return full, bounds


# ---- (b) narrow backward -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", SLOPES)
@pytest.mark.parametrize("B,K,L", BWD_SHAPES)
def test_narrow_backward(B, K, L, a):
    """coskad_btlnk_bwd_f32 at L <= 16 (k_btlnk_bwd, k_btlnk_reduce): k_du, k_dw, k_db, k_da_narrow with the chunk length of
    kernel_refs.btl_chunks; S dW slabs, B clips and ceil(K / 256) S slope partials are summed in double.  The workspace arrives as
    NaN, so a chunk past the batch that left its slab unwritten would show in dW."""
    pre = a is not None
    S, chunk = R.btl_chunks(B, K)
    d = R.btlnk_inputs(B, K, L, seed=B + K + L)
    dev = {k: v.cuda() for k, v in d.items()}
    s = _slope_dev(a)
    ref, M = _bwd_ref(d, a)
    ks_of = lambda acc: dict(dU=k_du(L, pre), dW=k_dw(chunk, pre, acc), db=k_db(acc), dslope=k_da_narrow(L, chunk, acc))
    counts = dict(dW=S, db=B, dslope=ceil_div(K, 256) * S)
    _bwd_modes(f"bwd {B}x{K}x{L} a={a}", lambda acc, absent, keep: _call_bwd(dev, s, B, K, L, acc, absent, keep), ref, M, ks_of, counts,
               pre)


# ---- (c) chain backward --------------------------------------------------------------------------------------------------------------

def _chain_inputs(B, TV, Ci, L, seed):
    d = R.btlnk_inputs(B, HID * TV, L, seed, TV=TV)
    g = torch.Generator().manual_seed(seed + 1)
    d["x_in"] = torch.randn(B, Ci, TV, generator=g)
    d["Z"] = torch.randn(B, Ci, TV, generator=g) * 1.5 - 0.25
    return d


def _call_chain(dev, s, s_in, B, TV, Ci, L, accumulate, absent=(), keep_slope=False):
    lib = _lib()
    K = HID * TV
    fill = PRIOR if accumulate else float("nan")
    nchain = lib.lib().coskad_btlnk_bwd_chain_floats(B, TV, Ci)
    bufs = {"dU": _out((B, K), float("nan")), "dW": _out((L, K), fill), "db": _out((L,), fill),
            "dslope": _out((1,), KEEP if keep_slope else fill), "chain": _out((nchain,), SENT)}
    arg = {k: (None if k in absent else v[1]) for k, v in bufs.items()}
    nbytes = lib.lib().coskad_btlnk_bwd_chain_ws_bytes(B, K, L, TV)
    ws = _scratch(nbytes)
    rows = ctypes.c_int(0)
    lib.call("coskad_btlnk_bwd_chain_f32", dev["U"], dev["W"], dev["dz"], s, arg["dU"], arg["dW"], arg["db"], arg["dslope"], ws, nbytes,
             1 if accumulate else 0, B, K, L, dev["x_in"], dev["Z"], s_in, Ci, TV, arg["chain"], nchain * 4, ctypes.byref(rows), _stream())
    for k, (buf, _) in bufs.items():
        _guards_intact(buf, "chain " + k)
    out = {k: v[1] for k, v in bufs.items()}
    out["rows"] = rows.value
    return out


@pytest.mark.parametrize("a", CHAIN_SLOPES)
@pytest.mark.parametrize("B,TV,Ci,L", CHAIN_SHAPES)
def test_chain_backward(B, TV, Ci, L, a):
    """coskad_btlnk_bwd_chain_f32 (k_btlnk_bwd_stats<1 / 2, false>, k_btlnk_reduce) with and without the input's slope.  Gradients:
    k_du, k_dw, k_db, k_da_chain with bc::plan's chunk; S slabs, B clips, `rows` slope partials in double; the modes of _bwd_modes;
    and the four agree with coskad_btlnk_bwd_f32 on the same inputs within the sum of the two bounds.  P / Q / s of ops.chain_sums
    against kernel_refs.top_layer_sums in double on the kernel's own dU read back (the kernel contracts the float32 tile it
    stores; dU itself is held to float64 above): k_chain_pq, k_chain_s, `rows` rows in double.  The float32 partial rows summed in
    double by the test equal chain_sums to (rows + 8) U64 M.  The repeat call's chain buffer is compared as int32 words."""
    from coskad_amd import ops
    pre = a is not None
    K = HID * TV
    npt, S, chunk = R.chain_plan(B, TV)
    rows = npt * S
    assert rows == _lib().lib().coskad_btlnk_bwd_chain_rows(B, TV)
    d = _chain_inputs(B, TV, Ci, L, seed=B + TV + Ci + L)
    dev = {k: v.cuda() for k, v in d.items()}
    s = _slope_dev(a)
    ref, M = _bwd_ref(d, a)
    ks_of = lambda acc: dict(dU=k_du(L, pre), dW=k_dw(chunk, pre, acc), db=k_db(acc), dslope=k_da_chain(L, chunk, acc))
    counts = dict(dW=S, db=B, dslope=rows)
    E = 2 * HID * Ci + HID
    Z64, x64 = dd(d["Z"]), dd(d["x_in"])
    first = None
    for a_in in IN_SLOPES:
        s_in = _slope_dev(a_in)
        tag = f"chain {B}x{TV}x{Ci}x{L} a={a} in={a_in}"
        call = lambda acc, absent, keep: _call_chain(dev, s, s_in, B, TV, Ci, L, acc, absent, keep)
        if first is None:
            out, bounds = _bwd_modes(tag, call, ref, M, ks_of, counts, pre)
            first = out
            again = call(False, (), not pre)
            assert _bits(again["chain"], out["chain"]), "chain buffer of a repeat call"
            narrow = _call_bwd(dev, s, B, K, L, False, (), not pre)
            nS, nchunk = R.btl_chunks(B, K)
            nb = dict(dU=_bd(k_du(L, pre), M["dU"]), dW=_bd(k_dw(nchunk, pre, False), M["dW"], nS), db=_bd(k_db(False), M["db"], B))
            if pre:
                nb["dslope"] = _bd(k_da_narrow(L, nchunk, False), M["dslope"], ceil_div(K, 256) * nS)
            for q in nb:
                gap = _np(out[q]).astype(np.float64) - _np(narrow[q])
                _close(f"{tag} {q} chain - narrow", gap, np.zeros_like(gap), bounds[q] + nb[q])
        else:
            out = call(False, (), not pre)
            for q in ("dU", "dW", "db", "dslope"):
                assert _bits(out[q], first[q]), (tag, q)            # the gradients do not depend on the input's slope
        assert out["rows"] == rows
        # P / Q / s
        dUk = dd(out["dU"]).view(B, HID, TV)
        P, Q, sv = R.top_layer_sums(dUk, Z64, x64, _slope_ref(a_in))
        X = x64 if a_in is None else R.prelu(x64, R.f32(a_in))
        MP, MQ, Ms = R.top_layer_sums(dUk.abs(), Z64.abs(), X.abs(), None)
        sums = ops.chain_sums(out["chain"], rows, Ci, HID).cpu()
        assert sums.dtype == torch.float64 and sums.numel() == E
        nPQ = HID * Ci
        _close(tag + " P", sums[:nPQ].numpy(), _np(P).ravel(), _bd(k_chain_pq(chunk, False), _np(MP).ravel(), rows))
        _close(tag + " Q", sums[nPQ:2 * nPQ].numpy(), _np(Q).ravel(), _bd(k_chain_pq(chunk, a_in is not None), _np(MQ).ravel(), rows))
        _close(tag + " s", sums[2 * nPQ:].numpy(), _np(sv), _bd(k_chain_s(chunk), _np(Ms), rows))
        part = dd(out["chain"][:rows * E]).view(rows, E)
        _close(tag + " rows summed", sums.numpy(), _np(part.sum(0)), (rows + 8) * U64 * _np(part.abs().sum(0)))


# ---- (d) the riding head --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("upstream", [1.0, 0.37])
@pytest.mark.parametrize("B,TV,Ci,L", RIDE_SHAPES)
def test_riding_head_at_other_windows(B, TV, Ci, L, upstream):
    """coskad_btlnk_bwd_chain_head_f32 against coskad_btlnk_fwd_ws_f32 + coskad_mse_head_f32 + coskad_btlnk_bwd_chain_f32, the
    comparison of test_gpu_head_rides.py (bit-equal on every output) at T V = 20 and 600 (nwg < 8 and a last position tile of 4;
    two tiles per workgroup) and with two head blocks behind 140 backward workgroups, at an upstream other than 1."""
    from coskad_amd import engine, ops
    K = HID * TV
    d = _chain_inputs(B, TV, Ci, L, seed=3 * B + TV + Ci + L)
    g = torch.Generator().manual_seed(B)
    dev = {k: v.cuda() for k, v in d.items()}
    U4, x4, Z4 = dev["U"].view(B, HID, 1, TV), dev["x_in"].view(B, Ci, 1, TV), dev["Z"].view(B, Ci, 1, TV)
    c = (torch.randn(L, generator=g) * 0.3).cuda()
    slope, in_slope = _slope_dev(0.3), _slope_dev(0.2)
    S = ops.head_slots(L)
    for accumulate, fill in ((False, float("nan")), (True, 0.25)):
        res = []
        for ride in (False, True):
            ws = engine.Workspace()
            dW, db, da = (torch.full(sh, fill, device="cuda") for sh in ((L, K), (L,), (1,)))
            acc = torch.full((S,), 0.125, device="cuda")
            if ride:
                part = ops.btlnk_fwd_parts(dev["U"], dev["W"], slope)
                z, dz, score, stats, dU, (chain, rows) = ops.btlnk_bwd_chain_head(
                    U4, dev["W"], part, dev["b"], c, slope, dW, db, da, ws, x4, Z4, in_slope, acc=acc, need_score=True, upstream=upstream,
                    accumulate=accumulate)
            else:
                z = ops.btlnk_fwd(dev["U"], dev["W"], dev["b"], slope, ws=ws)
                stats, dz, score = ops.mse_head(z, c, need_score=True, acc=acc, upstream=upstream)
                dU, (chain, rows) = ops.btlnk_bwd_chain(U4, dev["W"], dz, slope, dW, db, da, ws, x4, Z4, in_slope, accumulate=accumulate)
            res.append(dict(z=z, dz=dz, score=score, stats=stats, acc=acc, dU=dU, dW=dW, db=db, dslope=da, rows=rows,
                            sums=ops.chain_sums(chain, rows, Ci, HID), part=chain[:rows * (2 * HID * Ci + HID)]))
        want, got = res
        assert got["rows"] == want["rows"] == R.chain_plan(B, TV)[0] * R.chain_plan(B, TV)[1]
        for k in ("z", "dz", "score", "stats", "acc", "dU", "dW", "db", "dslope", "sums", "part"):
            assert _bits(got[k], want[k]), (k, accumulate)
        assert bool(torch.isfinite(got["dW"]).all()) and bool(torch.isfinite(got["stats"]).all())


# ---- (e) wide ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", SLOPES)
@pytest.mark.parametrize("B,K,L", WIDE_SHAPES)
def test_wide_forward_and_backward(B, K, L, a):
    """csrc/btlnk_wide.hip through coskad_btlnk_fwd_ws_f32 / coskad_btlnk_bwd_f32 at 16 < L <= 512.  Forward: k_fwd_wide, with and
    without a bias, a repeat call and every batch of FWD_SUBSETS below B bit-equal to the leading rows.  Backward: k_du; k_dw with
    bw::dw_chunk (at most B clips); k_db; k_da_wide; dw_chunks slabs, B clips and dx_blocks slope partials in double; the modes of
    _bwd_modes."""
    pre = a is not None
    d = R.btlnk_inputs(B, K, L, seed=B + K + L)
    dev = {k: v.cuda() for k, v in d.items()}
    s = _slope_dev(a)
    U, W = dd(d["U"]), dd(d["W"])
    X = U if a is None else R.prelu(U, R.f32(a))
    for bias in (True, False):
        b = dd(d["b"]) if bias else None
        zr = R.btlnk(U, _slope_ref(a), W, b)
        M = X.abs() @ W.abs().T + (b.abs() if bias else 0.0)
        z = _call_fwd_ws(dev, s, bias, B, K, L)
        _close(f"wide fwd {B}x{K}x{L} a={a} bias={bias}", _np(z), _np(zr), k_fwd_wide(K, L, pre, bias) * U32 * _np(M))
        assert _bits(_call_fwd_ws(dev, s, bias, B, K, L), z)
        for m in FWD_SUBSETS:
            if m < B:
                assert _bits(_call_fwd_ws(dev, s, bias, m, K, L), z[:m]), ("batch independence", m)
    ref, Mg = _bwd_ref(d, a)
    chunk = min(R.wide_dw_chunk(B, K, L), B)
    ks_of = lambda acc: dict(dU=k_du(L, pre), dW=k_dw(chunk, pre, acc), db=k_db(acc), dslope=k_da_wide(L, acc))
    counts = dict(dW=R.wide_dw_chunks(B, K, L), db=B, dslope=R.wide_dx_blocks(B, K))
    _bwd_modes(f"wide bwd {B}x{K}x{L} a={a}", lambda acc, absent, keep: _call_bwd(dev, s, B, K, L, acc, absent, keep), ref, Mg, ks_of,
               counts, pre)
