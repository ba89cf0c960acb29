"""The float64 references of kernel_refs.py against torch.nn / torch.optim on the CPU, before a device sees them: what the GPU
kernel tests (test_gpu_wide_kernels.py, test_gpu_narrow_conv.py, test_gpu_flat_kernels.py, test_gpu_head_kernels.py,
test_gpu_btlnk_kernels.py, test_gpu_decoder_kernels.py) compare with is shown right here, and the launch-plan restatements are held
against the library's host-only size queries; the running-error arithmetic behind the Poincare head's bounds against the oracle and numpy float32.  Also
the Python twin of the dropout hash (its keep rate; the numpy form against the integer form) and the share of elements the
apply / backward test leaves out at the PReLU kink, from the reference alone.  No kernel runs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
import test_gpu_wide_kernels as W

RTOL = 1e-11          # both sides are double: what is left is the order of summation


def _close(a, b, name):
    a, b = a.detach().numpy(), b.detach().numpy()
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=RTOL * max(1.0, float(np.abs(b).max())), err_msg=name)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("residual_bn", [True, False])
def test_bn2_block_is_batchnorm_add_prelu(training, residual_bn):
    """kernel_refs.bn2_block == nn.BatchNorm2d -> add -> nn.PReLU in double, outputs, every gradient and the running statistics"""
    g = torch.Generator().manual_seed(3 + int(training) + 2 * int(residual_bn))
    Nb, C, P, eps, mom = 6, 5, 11, 1e-5, 0.1
    Ct = (torch.randn(Nb, C, P, generator=g, dtype=torch.float64) * 1.7 + 0.6).requires_grad_(True)
    Cr = torch.randn(Nb, C, P, generator=g, dtype=torch.float64).requires_grad_(True)
    dOut = torch.randn(Nb, C, P, generator=g, dtype=torch.float64)
    bns = []
    for _ in range(2):
        bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).double()
        with torch.no_grad():
            bn.weight.copy_(torch.randn(C, generator=g)); bn.bias.copy_(torch.randn(C, generator=g))
            bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bns.append(bn.train(training))
    act = torch.nn.PReLU(init=0.1).double()
    rm0 = [bn.running_mean.clone() for bn in bns]
    rv0 = [bn.running_var.clone() for bn in bns]

    yr = bns[1](Cr[..., None]) if residual_bn else Cr[..., None]
    want = act(bns[0](Ct[..., None]) + yr)[..., 0]
    wp = [Ct, Cr, bns[0].weight, bns[0].bias, act.weight] + ([bns[1].weight, bns[1].bias] if residual_bn else [])
    wgrads = torch.autograd.grad(want, wp, dOut)

    leaf = lambda t: t.detach().clone().requires_grad_(True)
    t = dict(gamma=leaf(bns[0].weight), beta=leaf(bns[0].bias), running_mean=rm0[0], running_var=rv0[0])
    r = dict(gamma=leaf(bns[1].weight), beta=leaf(bns[1].bias), running_mean=rm0[1], running_var=rv0[1]) if residual_bn else None
    Ct2, Cr2, a2 = leaf(Ct), leaf(Cr), leaf(act.weight)
    got, u, (mean_t, inv_t), sr = R.bn2_block(Ct2, Cr2, t, r, a2, eps, training)
    gp = [Ct2, Cr2, t["gamma"], t["beta"], a2] + ([r["gamma"], r["beta"]] if residual_bn else [])
    ggrads = torch.autograd.grad(got, gp, dOut)
    _close(got, want, "out")
    assert torch.equal(R.prelu(u, a2), got)
    for k, (a, b) in enumerate(zip(ggrads, wgrads)):
        _close(a.reshape(-1), b.reshape(-1), f"grad {k}")
    for k, (x, bn) in enumerate(((Ct, bns[0]), (Cr, bns[1]))[:2 if residual_bn else 1]):
        if training:
            mean, var, inv = R.bn_batch_stats(x.detach(), eps)
            rm, rv = R.bn_running_update(mean, var, Nb * P, rm0[k], rv0[k], mom)
            _close(rm, bn.running_mean, "running_mean"); _close(rv, bn.running_var, "running_var")
            assert int(bn.num_batches_tracked) == 1
            if k == 0:
                _close(mean, mean_t, "mean"); _close(inv, inv_t, "invstd")
        else:
            assert torch.equal(bn.running_mean, rm0[k]) and torch.equal(bn.running_var, rv0[k]) and int(bn.num_batches_tracked) == 0
            if k == 0:
                assert torch.equal(mean_t, rm0[0])
                _close(inv_t, 1.0 / torch.sqrt(rv0[0] + eps), "invstd")


def test_bn2_block_mask_and_single_count():
    """the mask multiplies the tcn branch's BatchNorm output (nn.Dropout's place, stsgcn.py:66); a count of 1 keeps the biased variance
    in the running update (the `count > 1` guard)"""
    g = torch.Generator().manual_seed(11)
    Nb, C, P, eps = 4, 3, 9, 1e-5
    Ct, Cr = torch.randn(Nb, C, P, generator=g, dtype=torch.float64), torch.randn(Nb, C, P, generator=g, dtype=torch.float64)
    mask = (torch.rand(Nb, C, P, generator=g) < 0.75).double() / 0.75
    t = dict(gamma=torch.randn(C, generator=g, dtype=torch.float64), beta=torch.randn(C, generator=g, dtype=torch.float64))
    got, _, _, _ = R.bn2_block(Ct, Cr, t, None, 0.1, eps, True, mask)
    want = F.prelu(mask * F.batch_norm(Ct, None, None, t["gamma"], t["beta"], True, 0.0, eps) + Cr, torch.tensor([0.1], dtype=torch.float64))
    _close(got, want, "masked")
    x = torch.tensor([[[2.5]]], dtype=torch.float64)
    mean, var, inv = R.bn_batch_stats(x, eps)
    rm, rv = R.bn_running_update(mean, var, 1, torch.tensor([1.0]), torch.tensor([2.0]), 0.1)
    assert float(var) == 0.0 and float(rm) == pytest.approx(0.9 + 0.25) and float(rv) == pytest.approx(1.8)


@pytest.mark.parametrize("pre", [True, False])
def test_narrow_conv_is_conv2d_of_prelu(pre):
    """kernel_refs.narrow_conv == F.conv2d(F.prelu(U), W[:, :, None, None]) with its gradients, exact +0.0 / -0.0 in U included (the
    derivative at zero is the slope's side in both)"""
    g = torch.Generator().manual_seed(5)
    B, Ci, J, T, V = 3, 5, 4, 2, 7
    U = torch.randn(B, Ci, T, V, generator=g, dtype=torch.float64)
    U.view(-1)[0], U.view(-1)[1], U.view(-1)[17] = 0.0, -0.0, 0.0
    Wm = torch.randn(J, Ci, generator=g, dtype=torch.float64)
    dOut = torch.randn(B, J, T, V, generator=g, dtype=torch.float64)
    res = []
    for ref in (True, False):
        u, w, a = U.clone().requires_grad_(True), Wm.clone().requires_grad_(True), torch.tensor([0.2], dtype=torch.float64, requires_grad=True)
        if ref:
            out = R.narrow_conv(u.view(B, Ci, T * V), a if pre else None, w).view(B, J, T, V)
        else:
            out = F.conv2d(F.prelu(u, a) if pre else u, w[:, :, None, None])
        res.append((out,) + torch.autograd.grad(out, [u, w] + ([a] if pre else []), dOut))
    for k, (x, y) in enumerate(zip(*res)):
        _close(x.reshape(-1), y.reshape(-1), f"narrow {k}")
    if pre:
        assert float(res[0][1].view(-1)[0]) == float(res[1][1].view(-1)[0]) != 0.0


def test_rec_head_is_mse_of_prelu():
    g = torch.Generator().manual_seed(6)
    U, x = torch.randn(50, generator=g, dtype=torch.float64), torch.randn(50, generator=g, dtype=torch.float64)
    a = torch.tensor([0.15], dtype=torch.float64)
    assert float(R.rec_head(U, x, a)) == pytest.approx(float(F.mse_loss(F.prelu(U, a), x)), rel=1e-13)


def test_adam_step_is_torch_adam():
    """kernel_refs.adam_step == torch.optim.Adam in double over five steps; with the regulariser folded in, torch gets the folded
    gradient g gscale + reg_coef mask p"""
    g = torch.Generator().manual_seed(7)
    n, lr, b1, b2, eps = 40, 1e-3, 0.9, 0.999, 1e-8
    for mask, gscale, reg in ((None, 1.0, 0.0), ((torch.rand(n, generator=g) < 0.5).double().numpy(), 0.5, 1e-3)):
        p_t = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True)
        opt = torch.optim.Adam([p_t], lr=lr, betas=(b1, b2), eps=eps)
        p, m, v = p_t.detach().numpy().copy(), np.zeros(n), np.zeros(n)
        for t in range(1, 6):
            grad = torch.randn(n, generator=g, dtype=torch.float64)
            folded = grad * gscale + reg * (torch.from_numpy(mask) if mask is not None else 1.0) * p_t.detach()
            p_t.grad = folded.clone()
            opt.step()
            p, m, v = R.adam_step(p, grad.numpy(), m, v, t, lr, b1, b2, eps, mask, gscale, reg)
            np.testing.assert_allclose(p, p_t.detach().numpy(), rtol=1e-12, atol=1e-14)
            st = opt.state[p_t]
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-16)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-18)


def test_gather_transform_reference_is_the_einsum():
    """kernel_refs.gather_transform_f32 on valid indices against the reference formula einsum('ktv,ck->ctv', (x, y, 1), M) in double"""
    rng = np.random.default_rng(0)
    N, ntrans, TV = 4, 3, 6
    xy, mats = rng.standard_normal((N, 2, TV)).astype(np.float32), rng.standard_normal((ntrans, 3, 3)).astype(np.float32)
    idx = [0, 5, N * ntrans - 1, -1, N * ntrans]
    got = R.gather_transform_f32(xy, mats, idx, N, ntrans)
    for b, i in enumerate(idx):
        if i < 0 or i // N >= ntrans:
            assert not got[b].any()
            continue
        h = np.concatenate([xy[i % N].astype(np.float64), np.ones((1, TV))])
        want = np.einsum("kp,ck->cp", h, mats[i // N].astype(np.float64))[:2]
        M = np.abs(mats[i // N, :2]).astype(np.float64) @ np.abs(h)          # two products, two adds: k = 4 at most
        assert np.all(np.abs(got[b] - want) <= 4 * R.U32 * M)


@pytest.mark.parametrize("seed", R.DROP_SEEDS)
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_twin_keep_rate(p, seed):
    """the share of kept elements is within 3 sigma of 1 - p at the size and seeds of the GPU test; kept values are 1 / (1 - p) in
    float32; p = 0 keeps everything"""
    n = 70_000
    m = R.drop_mask_twin(n, p, seed)
    kept = float((m > 0).mean())
    assert abs(kept - (1 - p)) <= 3 * np.sqrt(p * (1 - p) / n), kept
    assert set(np.unique(m)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    assert np.array_equal(R.drop_mask_twin_np(n, p, seed), m)
    assert np.array_equal(R.drop_mask_twin(100, 0.0, seed), np.ones(100, np.float32))


# ---- the one-class heads: the restated Poincare chain and its running-error arithmetic ---------------------------------------------------

HEAD_LS = [1, 2, 5, 16, 17, 65, 512]


def _head_case(L, cnorm, B=67):
    """float32 inputs of kernel_refs.head_inputs with the oracle's double forward and autograd gradient on them"""
    from oracle import ref_cpu as O
    z, c = R.head_inputs(B, L, cnorm if cnorm is not None else 0.4, seed=3)
    zd = z.double().requires_grad_(True)
    loss, zh = O.poincare_loss(zd, c.double())
    (gz,) = torch.autograd.grad(loss, zd)
    return z, c, zh.detach(), O.dist(c.double()[None], zh.detach()), gz, O


@pytest.mark.parametrize("cnorm", R.HEAD_CENTRES)
@pytest.mark.parametrize("L", HEAD_LS)
def test_head_chain_in_double_is_the_oracle(L, cnorm):
    """the restated kernel sequences (kernel_refs.poincare_head_chain, logmap0_chain), evaluated in double, equal oracle/ref_cpu.py's
    project(expmap0(z)), dist and logmap0 to 1e-12, their hand-written backward equals autograd on the oracle's forward, the slot sums
    give the oracle's gyromidpoint, and the oracle's gradients are finite on every row -- at both dot-product orders"""
    z, c, zh, d, gz, O = _head_case(L, cnorm)
    B = z.shape[0]
    assert torch.isfinite(gz).all() and torch.isfinite(d).all()
    for wide in (False, True):
        A = R.EVMath()
        out = R.poincare_head_chain(A, z, c, wide, R.gscale_pair(1.0, B))
        tol = lambda ref: 1e-12 * max(1.0, float(ref.abs().max()))
        assert float((out["zh"].v - zh).abs().max()) <= tol(zh)
        # two double evaluations of |m| differ by a few roundings, which artanh amplifies by 2 / (1 - mc^2) (up to 1e5 at the clamp):
        # eight of them on top of the 1e-12
        amp = 2.0 / (1.0 - torch.tanh(d / 2) ** 2)
        assert bool(((out["d"].v[:, 0] - d).abs() <= 1e-12 * d.abs().clamp_min(1.0) + 8 * R.U64 * amp).all())
        # the backward is a restatement too (it only supplies the bound): rows at the ball's edge amplify double rounding by 1 / (1 - mn^2)
        assert float((out["dz"].v - gz).abs().max()) <= 1e-9 * float(gz.abs().max())
        S, s, nb = R.poincare_slot_sums(zh)
        assert float((out["gzh"].v.sum(0) - S).abs().max()) <= 1e-12 * float(S.abs().max())
        assert float((out["gm1"].v.sum() - s).abs()) <= 1e-12 * float(s) and float((out["norm"].v.sum() - nb).abs()) <= 1e-12 * float(nb)
        mid = O.weighted_midpoint(zh)
        assert float((R.midpoint_from_sums(S, s) - mid).abs().max()) <= 1e-12
        lm = R.logmap0_chain(A, zh.float(), wide)
        want = O.logmap0(zh.float().double())
        assert float((lm.v - want).abs().max()) <= tol(want)


@pytest.mark.parametrize("cnorm", R.HEAD_CENTRES)
@pytest.mark.parametrize("L", HEAD_LS)
def test_head_chain_in_float32_lies_within_the_running_error_bound(L, cnorm):
    """the same sequences in numpy float32 (every operation rounded, fmaf rounded once, the kernels' summation orders) lie within the
    arithmetic's bound of the double value, for every output of the head; and no row lies nearer to a select's threshold (projection,
    min-norm, tanh clamp) than the compared quantity's bound: the cap on rows left out is 0.  (The artanh clamp is no select: a
    minimum is continuous and Artanh.backward takes the clamped value on both sides, so its error passes through EV.minimum.)"""
    z, c, zh, d, gz, O = _head_case(L, cnorm)
    B = z.shape[0]
    for wide in ((False, True) if L <= R.HEAD_LMAX else (True,)):         # the one-thread chain of L fmaf exists up to L = 16 only
        A, F = R.EVMath(), R.F32Math()
        gs = R.gscale_pair(0.37, B)
        ev = R.poincare_head_chain(A, z, c, wide, gs)
        fl = R.poincare_head_chain(F, z, c, wide, gs)
        for name, margin, bound in A.margins:
            assert bool((margin > bound).all()), (name, float((margin - bound).min()))
        for k in ("zh", "d", "dz", "gzh", "gm1", "norm"):
            err = (F.value(fl[k]) - ev[k].v).abs()
            ratio = float((err / ev[k].e.clamp_min(1e-300)).max())
            assert torch.isfinite(ev[k].e).all() and ratio <= 1.0, (k, wide, ratio)
        y = zh.float()
        le, lf = R.logmap0_chain(A, y, wide), R.logmap0_chain(F, y, wide)
        assert float(((F.value(lf) - le.v).abs() / le.e.clamp_min(1e-300)).max()) <= 1.0


def test_euclid_slot_sums_give_the_oracle_centre():
    from oracle import ref_cpu as O
    z = torch.randn(37, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 1e-2
    S, n, nb, G = R.euclid_slot_sums(z)
    assert n == 37 and torch.allclose(G, torch.einsum("ni,nj->ij", z, z), rtol=1e-13, atol=1e-16)
    assert torch.equal(O.clamp_center(S / n, 1e-3), O.clamp_center(z.sum(0) / 37, 1e-3)) and float(nb) == pytest.approx(float(z.norm(dim=1).sum()))


@pytest.mark.parametrize("Nb,C,P", W.APPLY_SHAPES)
def test_kink_share_of_the_reference_alone(Nb, C, P):
    """the apply / backward test leaves out the elements whose double u lies within the float32 rounding bound of zero; with the
    reference's own u their share is far below the test's cap of 1e-3 at every shape and configuration it runs (the dropout cases with
    the twin's mask at the case's seed, whose keep rate is within 3 sigma of 0.75)"""
    for residual_bn in (True, False):
        for training, drop_p in ((True, 0.0), (True, 0.25), (False, 0.0)):
            def mask_fn(shape, p, seed):
                m = R.drop_mask_twin_np(int(np.prod(shape)), p, seed)
                assert abs(float((m > 0).mean()) - (1 - p)) <= 3 * np.sqrt(p * (1 - p) / m.size)
                return torch.from_numpy(m).view(shape)
            k = W._apply_case(Nb, C, P, residual_bn, training, drop_p, mask_fn)
            share = float(k["kink"].double().mean())
            assert share <= 1e-3, (residual_bn, training, drop_p, share)
            assert torch.isfinite(k["out_ref"]).all() and all(torch.isfinite(g).all() for g in k["grads"].values())


# ---- the bottleneck: references, input builder, launch-plan restatements, and the edge every test shape is listed for -------------------

@pytest.mark.parametrize("a", [None, 0.25, 0.0, -0.5, 1.0])
def test_btlnk_is_linear_of_prelu(a):
    """kernel_refs.btlnk == nn.Linear(nn.PReLU(U)) in double, z and every gradient, on kernel_refs.btlnk_inputs (exact +0.0 / -0.0 in U:
    the derivative at zero is the slope's side in both); slope None: the Linear alone; without a bias too"""
    B, K, L = 19, 36, 5
    d = R.btlnk_inputs(B, K, L, seed=4)
    dz = d["dz"].double()
    res = []
    for ref in (True, False):
        U, Wm, b = (d[k].double().clone().requires_grad_(True) for k in ("U", "W", "b"))
        s = None if a is None else torch.tensor([a], dtype=torch.float64, requires_grad=True)
        if ref:
            z = R.btlnk(U, s, Wm, b)
        else:
            z = F.linear(U if a is None else F.prelu(U, s), Wm, b)
        res.append((z,) + torch.autograd.grad(z, [U, Wm, b] + ([] if a is None else [s]), dz))
    for k, (x, y) in enumerate(zip(*res)):
        _close(x.reshape(-1), y.reshape(-1), f"btlnk {k}")
    n0, k0 = R.btlnk_zero_plants(B, K)[0]
    if a is not None:
        assert float(res[0][1][n0, k0]) == float(res[1][1][n0, k0]) == a * float((dz @ d["W"].double())[n0, k0])
    U, Wm = d["U"].double(), d["W"].double()
    _close(R.btlnk(U, None, Wm, None), F.linear(U, Wm), "no bias")


@pytest.mark.parametrize("a_in", [None, 0.2])
def test_top_layer_sums_are_the_weight_gradients(a_in):
    """kernel_refs.top_layer_sums == autograd of sum dU (Wz Z + Wx PReLU(x) + bias) with respect to Wz, Wx and the bias"""
    g = torch.Generator().manual_seed(12)
    B, Co, Ci, TV = 5, 6, 3, 11
    dU, Z, x = (torch.randn(B, c, TV, generator=g, dtype=torch.float64) for c in (Co, Ci, Ci))
    Wz, Wx = (torch.randn(Co, Ci, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    bias = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    X = x if a_in is None else F.prelu(x, torch.tensor([a_in], dtype=torch.float64))
    out = torch.einsum("oc,ncp->nop", Wz, Z) + torch.einsum("oc,ncp->nop", Wx, X) + bias[None, :, None]
    want = torch.autograd.grad((dU * out).sum(), [Wz, Wx, bias])
    for k, (x_, y_) in enumerate(zip(R.top_layer_sums(dU, Z, x, a_in), want)):
        _close(x_.reshape(-1), y_.reshape(-1), f"sums {k}")


@pytest.mark.parametrize("B,K,TV", [(1, 4, None), (1, 3, None), (17, 260, None), (100, 64 * 600, 600), (33, 64 * 20, 20)])
def test_btlnk_inputs_plants_and_magnitudes(B, K, TV):
    """the planted elements are exact zeros of alternating sign; first, second, middle and last element, one element of the last clip
    of every 16-clip tile and one in the last position tile are among them; nothing else is zero, nothing is subnormal; the three
    magnitudes all occur"""
    d = R.btlnk_inputs(B, K, 5, seed=1, TV=TV)
    U = d["U"]
    spots = R.btlnk_zero_plants(B, K, TV)
    assert int((U == 0).sum()) == len(spots) <= max(1, B * K // 4)
    for i, (n, k) in enumerate(spots):
        assert float(U[n, k]) == 0.0 and bool(torch.signbit(U[n, k])) == bool(i % 2)
    if B * K >= 64:
        flat = {n * K + k for n, k in spots}
        assert {0, 1, B * K // 2, B * K - 1} <= flat
        tv = K if TV is None else TV
        for t in range(R.ceil_div(B, 16)):
            row = min(16 * t + 15, B - 1)
            cols = [k for n, k in spots if n == row]
            assert cols and any(k % tv >= 16 * ((tv - 1) // 16) for k in cols), t
        a = U.abs()
        assert bool((a[a > 0] >= R.F32_TINY).all()) and float(a.max()) > 30.0 and 0 < float(a[a > 0].min()) < 1e-3
    assert tuple(d["W"].shape) == (5, K) and tuple(d["dz"].shape) == (B, 5) and tuple(d["b"].shape) == (5,)


def _library():
    from coskad_amd import _lib
    return _lib.lib()


def test_btlnk_plan_restatements_match_the_library():
    """kernel_refs.btl_chunks, chain_plan, wide_fwd_slices, wide_dw_chunks, wide_dx_blocks against the library's pure-host size queries
    (no device is touched), at every shape of test_gpu_btlnk_kernels.py and over a grid of others"""
    import test_gpu_btlnk_kernels as BK
    lib = _library()
    KS = lib.coskad_btlnk_fwd_ks()
    assert 1 <= KS <= 8
    narrow = list(BK.BWD_SHAPES) + [(B, K, L) for B in (1, 16, 17, 300, 1024, 1025, 4096) for K in (4, 252, 256, 260, 816, 13056, 26112)
                                    for L in (1, 9, 16)]
    for B, K, L in narrow:
        assert lib.coskad_btlnk_bwd_ws_bytes(B, K, L) == 4 * R.btl_bwd_ws_floats(B, K, L), (B, K, L)
        assert lib.coskad_btlnk_fwd_ws_bytes_l(B, K, L) == 4 * KS * B * 16
        S, chunk = R.btl_chunks(B, K)
        assert 1 <= S <= 64 and chunk % 16 == 0 and S * chunk >= B
    chain = [(B, TV, Ci, L) for B, TV, Ci, L in BK.CHAIN_SHAPES + BK.RIDE_SHAPES]
    chain += [(B, TV, Ci, 16) for B in (1, 16, 17, 255, 256, 257, 4096) for TV in (4, 16, 136, 204, 272, 300, 408, 600) for Ci in (16, 32)]
    for B, TV, Ci, L in chain:
        npt, S, chunk = R.chain_plan(B, TV)
        K = 64 * TV
        assert lib.coskad_btlnk_bwd_chain_ok(K, TV, Ci) == 1
        assert lib.coskad_btlnk_bwd_chain_rows(B, TV) == npt * S, (B, TV)
        assert lib.coskad_btlnk_bwd_chain_ws_bytes(B, K, L, TV) == 4 * (S * L * K + S * npt + 64)
        assert lib.coskad_btlnk_bwd_chain_floats(B, TV, Ci) == R.chain_floats(B, TV, Ci)
        assert chunk % 16 == 0 and (S - 1) * chunk < B <= S * chunk             # the chain kernel has no empty chunk
    wide = list(BK.WIDE_SHAPES) + [(B, K, L) for B in (1, 128, 129, 1025, 4096) for K in (3, 128, 129, 1030, 13056) for L in (17, 32, 33, 64,
                                                                                                                         65, 128, 129, 512)]
    for B, K, L in wide:
        assert lib.coskad_btlnk_fwd_ws_bytes_l(B, K, L) == 4 * R.wide_fwd_slices(K, L) * B * L, (B, K, L)
        assert lib.coskad_btlnk_bwd_ws_bytes(B, K, L) == 4 * (R.wide_dw_chunks(B, K, L) * L * K + R.wide_dx_blocks(B, K) + 64), (B, K, L)
        assert R.wide_fwd_rchunk(K, L) % 16 == 0 and R.wide_dw_chunk(B, K, L) % 16 == 0


def test_btlnk_shapes_meet_the_edges_they_are_listed_for():
    """every shape of test_gpu_btlnk_kernels.py, from the plan restatements alone (held to the library above): a later change of a
    launcher that moves a case off its edge fails here"""
    import test_gpu_btlnk_kernels as BK
    cd = R.ceil_div
    # (a) direct forward: k-steps over eight waves
    steps = [cd(K, 16) for K in BK.FWD_K_DIRECT]
    assert steps == [1, 2, 3, 17, 52]
    assert [K % 16 for K in BK.FWD_K_DIRECT] == [4, 4, 0, 0, 4]                          # the k < K tail, and K = 4: one lane group
    per = [cd(s, 8) for s in steps]
    assert [sum(1 for w in range(8) if w * p >= s) for p, s in zip(per, steps)] == [7, 6, 5, 2, 0]       # empty waves
    assert per[3] % 4 and per[4] % 4                                                      # a partly filled batch of UB = 4 k-steps
    assert set(BK.FWD_BS) >= {1, 15, 16, 17, 63, 64, 65, 130}
    # split-K forward: 16 wave groups, empty and odd-length slices
    G = 4 * _library().coskad_btlnk_fwd_ks()
    lens = {K: [K // 16 * (g + 1) // G - K // 16 * g // G for g in range(G)] for K in BK.FWD_K_SPLIT}
    assert [K // 16 for K in BK.FWD_K_SPLIT] == [1, 5, 17, 81] and all(K % 16 == 0 for K in BK.FWD_K_SPLIT)
    assert 0 in lens[16] and 0 in lens[80] and any(l % 2 for l in lens[272]) and any(l % 2 for l in lens[1296]) and min(lens[1296]) >= 5
    assert all(K < 256 for K in BK.FWD_K_SPLIT[:2])
    # (b) narrow backward
    plan = {s: R.btl_chunks(s[0], s[1]) for s in BK.BWD_SHAPES}
    assert plan[(1, 4, 1)] == (1, 16) and plan[(15, 20, 5)] == (1, 16)
    assert 260 % 256 == 4 and plan[(17, 260, 16)] == (2, 16)                            # a second column block of one lane
    assert plan[(100, 272, 15)] == (7, 16)                                              # fewer slabs than the unroll of eight
    S, chunk = plan[(330, 13056, 16)]
    assert S * chunk - 330 >= chunk                                                      # wholly empty chunks at the production K
    assert plan[(1041, 272, 16)] == (64, 32) and sum(1 for y in range(64) if y * 32 >= 1041) == 31
    S, chunk = plan[(1041, 1280, 5)]
    assert cd(1280, 256) * S == 320 > 256 and 1041 > 4 * 256                            # slope partials and clips per db thread column
    S, chunk = plan[(145, 272, 8)]
    assert S == 10 and S > 8 and S % 8                                                   # the dW slab loop's remainder behind one round
    # (c) chain backward
    cp = {s: R.chain_plan(s[0], s[1]) for s in BK.CHAIN_SHAPES}
    assert all(s[1] % 4 == 0 and s[2] in (16, 32) for s in BK.CHAIN_SHAPES)
    assert cp[(1, 4, 16, 1)] == (1, 1, 16)
    npt, S, chunk = cp[(17, 20, 32, 8)]
    assert npt * S == 4 < 8 and 20 - 16 * (npt - 1) == 4                                # nwg < 8; a last position tile of 4
    assert 136 - 16 * (cp[(37, 136, 16, 16)][0] - 1) == 8                               # a last position tile of 8
    assert 204 - 16 * (cp[(40, 204, 32, 16)][0] - 1) == 12
    npt, S, chunk = cp[(100, 600, 32, 16)]
    assert chunk == 32 and 100 - (S - 1) * chunk == 4 and npt * S > 128                 # two tiles per workgroup, a last chunk of 4
    assert cp[(700, 204, 32, 9)][2] == 48                                               # three tiles per workgroup
    npt, S, chunk = cp[(1120, 20, 16, 16)]
    assert npt * S == 140 and S == 70                                                    # the unrolled row sum (rows > 7 * 16) and slab sum
    npt, S, chunk = cp[(33, 272, 32, 5)]
    assert 272 % 16 == 0 and 33 - (S - 1) * chunk == 1
    assert {s[2] for s in BK.CHAIN_SHAPES} == {16, 32} and {s[3] for s in BK.CHAIN_SHAPES} >= {1, 5, 8, 9, 16}
    # (d) riding head: two head blocks behind the backward's workgroups
    assert R.head_blocks(600, 16) == 2 and R.head_blocks(100, 16) == 1
    # (e) wide
    assert {R.wide_tile(s[2]) for s in BK.WIDE_SHAPES} == {1, 2, 4}
    sl = {s: R.wide_fwd_slices(s[1], s[2]) for s in BK.WIDE_SHAPES}
    assert sl[(1, 3, 17)] == 1 and sl[(127, 100, 32)] == 1 and sl[(260, 100, 200)] == 1
    assert sl[(300, 272, 64)] == 3 and 272 - 2 * R.wide_fwd_rchunk(272, 64) == 80 < R.wide_fwd_rchunk(272, 64)       # the last slice ragged
    assert sl[(129, 1030, 65)] == 9 and 1030 % 4 == 2 and sl[(40, 129, 129)] == 2 and sl[(20, 272, 512)] == 3
    assert {s[0] for s in BK.WIDE_SHAPES} >= {127, 129} and {s[1] for s in BK.WIDE_SHAPES} >= {100, 129, 272}       # both sides of 128
    assert R.wide_dw_chunk(1040, 36, 40) == 32 and all(R.wide_dw_chunk(*s) == 16 for s in BK.WIDE_SHAPES[:-1])
    assert R.wide_dw_chunks(300, 272, 64) == 19 > 8 and R.wide_dx_blocks(300, 272) == 9


# ---- the decoder models' stand-alone kernels: rev_btlnk at latent 8 / 16, the fold, the mlp head ----------------------------------------

@pytest.mark.parametrize("bias", [True, False])
def test_rev_btlnk_is_linear(bias):
    """kernel_refs.rev_btlnk == F.linear in double; dz = dH W, dW = dH^T z, db = sum_b dH are autograd's"""
    d = R.rev_inputs(19, 36, 8, seed=2)
    z, Wm, b, dH = (d[k].double().clone().requires_grad_(True) for k in ("z", "W", "b", "dH"))
    H = R.rev_btlnk(z, Wm, b if bias else None)
    _close(H, F.linear(z, Wm, b if bias else None), "H")
    gz, gW = torch.autograd.grad(H, [z, Wm], dH.detach(), retain_graph=True)
    _close(gz, dH.detach() @ Wm.detach(), "dz"); _close(gW, dH.detach().T @ z.detach(), "dW")
    if bias:
        (gb,) = torch.autograd.grad(H, [b], dH.detach())
        _close(gb, dH.detach().sum(0), "db")


def test_rev_plan_restatement_matches_the_library():
    """kernel_refs.rev_slices against coskad_rev_btlnk_ws_floats(B, N, L) / (N (L + 1)) (a pure-host query) at every shape of
    test_gpu_decoder_kernels.py and over a grid of others"""
    import test_gpu_decoder_kernels as DK
    lib = _library()
    shapes = [(B, N, L) for B in DK.REV_BS for N in DK.REV_NS for L in DK.REV_LS] + [DK.REV_PROD]
    shapes += [(B, N, L) for B in (1, 15, 16, 31, 32, 255, 256, 257, 450, 1023, 1024, 4096, 5000) for N in (4, 1024, 1028, 13056, 19200, 38400,
                                                                                                        65536, 131072) for L in (8, 16)]
    for B, N, L in shapes:
        S = R.rev_slices(B, N)
        assert lib.coskad_rev_btlnk_ws_floats(B, N, L) == S * N * (L + 1), (B, N, L)
        assert 1 <= S <= 64 and (B < 16 or S <= B // 16)
        assert R.rev_fwd_slices(B, N) in (1, 4, S)


def test_rev_shapes_meet_the_edges_they_are_listed_for():
    """every N and B of test_gpu_decoder_kernels.py's rev_btlnk section, from the plan restatement alone"""
    import test_gpu_decoder_kernels as DK
    cd = R.ceil_div
    # N: one thread; under one column block; a second block of one thread (the others return at n >= N) and a second k_rev_dz stride
    # of one float4; the folded first layer's 32 x 204 columns
    assert DK.REV_NS == (4, 816, 1028, 6528) and all(N % 4 == 0 for N in DK.REV_NS)
    assert 4 // 4 == 1 and 816 // 4 < 256 and cd(1028 // 4, 256) == 2 and 1028 // 4 - 256 == 1 and 1028 - 1024 == 4 and 6528 == 32 * 204
    assert [cd(N, 1024) for N in DK.REV_NS] == [1, 1, 2, 7]
    # B: k_rev_dz's CB = 4 (L = 8) and CB = 2 (L = 16) with every remainder
    assert {B % 4 for B in DK.REV_BS} == {0, 1, 2, 3} and {B % 2 for B in DK.REV_BS} == {0, 1}
    for N in DK.REV_NS:
        sl = [R.rev_slices(B, N) for B in DK.REV_BS]
        assert sl == [1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 4, 63, 64, 64], (N, sl)
        S, chunk = 64, cd(1030, 64)
        assert sum(1 for y in range(S) if y * chunk >= 1030) == 3                        # wholly empty trailing slices
        assert [R.rev_fwd_slices(B, N) for B in (63, 64, 65, 1023, 1024, 1030)] == [1, 4, 4, 4, 64, 64]
    assert {1, 2, 3, 5, 15, 16, 17, 33, 63, 64, 65, 1023, 1024, 1030} == set(DK.REV_BS)
    B, N, L = DK.REV_PROD
    assert (B, N, L) == (450, 38400, 16) and R.rev_slices(B, N) == 27 and 16 < 27 < min(64, B // 16) and R.rev_fwd_slices(B, N) == 4


def _fold_real_op(d, Co, TV, eps, moms, X, with_bias):
    """the operation the fold stands for: the latents expanded through X into the layer's two branches, a conv bias on each, nn.BatchNorm2d
    in training mode in double on each, added -> (out [n, Co, TV], the modules)"""
    zt = d["zt"]
    out, bns = 0.0, []
    for r in range(2):
        bn = torch.nn.BatchNorm2d(Co, eps=R.f32(eps[r]), momentum=R.f32(moms[r])).double().train()
        with torch.no_grad():
            bn.weight.copy_(d[f"gamma{r}"]); bn.bias.copy_(d[f"beta{r}"])
            bn.running_mean.copy_(d[f"rmean{r}"]); bn.running_var.copy_(d[f"rvar{r}"])
        Hr = torch.einsum("nl,lcp->ncp", zt, X[r])
        if with_bias[r]:
            Hr = Hr + d[f"cbias{r}"].double()[None, :, None]
        out = out + bn(Hr[..., None])[..., 0]
        bns.append(bn)
    return out, bns


@pytest.mark.parametrize("n,Co,TV,with_bias", [(37, 2, 20, (True, True)), (1, 2, 7, (False, True)), (5, 1, 1, (True, False)),
                                               (37, 3, 20, (True, True))])
def test_fold_is_batchnorm_of_the_expanded_layer(n, Co, TV, with_bias):
    """kernel_refs.fold against the real operation in double: with G = zt^T zt and n_pos = n T V, zt [Mw | Mb] equals the sum of the two
    train-mode BatchNorm2d outputs of the expanded branches to 1e-12 of its scale, the running statistics equal the modules' (conv bias
    included, unbiased variance, per-branch momentum and eps), and the gradients with respect to X, gamma and beta through the
    expansion equal autograd's on the restatement.  Co = 2 has the all-zero branch (variance exactly 0 on both sides).  Co = 3 adds the
    channel whose constant image is 10^3 times its spread: there E2 - mean^2 cancels six digits in double itself, so that one case is
    held to 1e-12 times (E2 + mean^2) / (var + eps), the cancellation's own amplification."""
    eps, moms = (1e-5, 1e-3), (0.1, 0.3)
    d = R.fold_inputs(Co, TV, n, seed=7 * n + Co + TV)
    g = torch.Generator().manual_seed(n)
    dOut = torch.randn(n, Co, TV, generator=g, dtype=torch.float64)
    leaf = lambda t: t.double().clone().requires_grad_(True)
    res = []
    for real in (True, False):
        X = leaf(d["X"])
        gam, bet = [leaf(d["gamma0"]), leaf(d["gamma1"])], [leaf(d["beta0"]), leaf(d["beta1"])]
        if real:
            out, bns = _fold_real_op(d, Co, TV, eps, moms, X, with_bias)
            gam, bet = [bn.weight for bn in bns], [bn.bias for bn in bns]
        else:
            f = R.fold(X, d["G"], gam, bet, eps, d["n_pos"])
            out = torch.einsum("nl,cpl->ncp", d["zt"], torch.cat([f["Mw"], f["Mb"][..., None]], -1))
        res.append((out,) + torch.autograd.grad(out, [X] + gam + bet, dOut))
    f = {k: v.detach() for k, v in f.items()}
    amp = 1.0
    if Co >= 3:
        amp = float(((f["E2"] + f["mean"] ** 2) / (f["var"] + torch.tensor(eps, dtype=torch.float64)[:, None])).max())
        assert amp > 1e5
    for k, (a, b) in enumerate(zip(*res)):
        a, b = a.detach(), b.detach()
        tol = 1e-12 * amp * max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= tol, (k, float((a - b).abs().max()), tol)
    if Co >= 2:
        assert float(f["var"][0, 1]) == 0.0 and float(f["istd"][0, 1]) == pytest.approx(1 / np.sqrt(R.f32(eps[0])), rel=1e-15)
    for r in range(2):
        cb = d[f"cbias{r}"].double() if with_bias[r] else None
        rm, rv = R.fold_running(f["mean"][r].detach(), f["var"][r].detach(), d["n_pos"], cb, d[f"rmean{r}"].double(), d[f"rvar{r}"].double(),
                                moms[r])
        for got, want in ((rm, bns[r].running_mean), (rv, bns[r].running_var)):
            assert float((got - want).abs().max()) <= 1e-12 * amp * max(1.0, float(want.abs().max())), r
    # the per-channel copy of G: its gradient is the channel's share, and the shares add up to the gradient of the one G
    X = d["X"].double()
    gam, bet = [d["gamma0"].double(), d["gamma1"].double()], [d["beta0"].double(), d["beta1"].double()]
    dMw, dMb = d["dMw"].double(), d["dMb"].double()
    grads = []
    for per_channel in (True, False):
        Gl = (d["G"][None].expand(Co, 9, 9) if per_channel else d["G"]).clone().requires_grad_(True)
        f2 = R.fold(X, Gl, gam, bet, eps, d["n_pos"])
        loss = (f2["Mw"].reshape(Co * TV, 8) * dMw).sum() + (f2["Mb"].reshape(Co * TV) * dMb).sum()
        grads.append(torch.autograd.grad(loss, Gl)[0])
    assert float((grads[0].sum(0) - grads[1]).abs().max()) <= 1e-12 * amp * max(1.0, float(grads[1].abs().max()))


def test_fold_shapes_meet_the_edges_they_are_listed_for():
    """T V of test_gpu_decoder_kernels.py against the position rounds of k_fold_fwd / k_fold_bwd (256 threads, MAXPOS = 2), the
    library's own shape query on both sides of its limit, and n_pos = 1"""
    import test_gpu_decoder_kernels as DK
    lib = _library()
    rnd = R.FOLD_ROUND
    assert DK.FOLD_TVS == (1, 63, 136, 204, 256, 257, 300, 408, 512) and DK.FOLD_COS == (1, 3, 32) and DK.FOLD_NS == (1, 37)
    first = [min(TV, rnd) for TV in DK.FOLD_TVS]
    second = [max(TV - rnd, 0) for TV in DK.FOLD_TVS]
    assert first == [1, 63, 136, 204, 256, 256, 256, 256, 256] and second == [0, 0, 0, 0, 0, 1, 44, 152, 256]
    for TV in range(1, 2 * rnd + 40):
        assert lib.coskad_lowrank_fold_ok(R.FOLD_K - 1, TV) == int(TV <= 2 * rnd)
    assert min(DK.FOLD_NS) * min(DK.FOLD_TVS) == 1
    assert DK.FOLD_MOM[0] != DK.FOLD_MOM[1] and DK.FOLD_EPS[0] != DK.FOLD_EPS[1]
    assert {c["cbias"] for c in DK.FOLD_CFGS} == {(True, True), (False, True), (True, False), (False, False)}
    assert {c["run"] for c in DK.FOLD_CFGS} == {(True, True), (False, True), (True, False), (False, False)}


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_mlp_head_is_batchnorm1d_relu_linear(training, bias):
    """kernel_refs.mlp_head == nn.BatchNorm1d -> nn.ReLU -> nn.Linear in double: z, every gradient, the batch statistics and the
    running update (unbiased variance) in train mode; the running statistics in eval mode.  The inputs carry the planted features."""
    B, H, L, eps, mom = 37, 7, 5, 1e-5, 0.1
    d = R.mlp_inputs(B, H, L, seed=3)
    bn = torch.nn.BatchNorm1d(H, eps=R.f32(eps), momentum=R.f32(mom)).double()
    lin = torch.nn.Linear(H, L, bias=bias).double()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rmean"]); bn.running_var.copy_(d["rvar"])
        lin.weight.copy_(d["W2"])
        if bias:
            lin.bias.copy_(d["b2"])
    bn.train(training)
    dz = d["dz"].double()
    y = d["y"].double().clone().requires_grad_(True)
    want = lin(torch.relu(bn(y)))
    wp = [y, bn.weight, bn.bias, lin.weight] + ([lin.bias] if bias else [])
    wg = torch.autograd.grad(want, wp, dz)
    leaf = lambda t: t.double().clone().requires_grad_(True)
    y2, gam, bet, W2 = leaf(d["y"]), leaf(d["gamma"]), leaf(d["beta"]), leaf(d["W2"])
    b2 = leaf(d["b2"]) if bias else None
    f = R.mlp_head(y2, gam, bet, W2, b2, eps, training, d["rmean"].double(), d["rvar"].double())
    gg = torch.autograd.grad(f["z"], [y2, gam, bet, W2] + ([b2] if bias else []), dz)
    _close(f["z"], want, "z")
    for k, (a, b) in enumerate(zip(gg, wg)):
        _close(a.reshape(-1), b.reshape(-1), f"grad {k}")
    if training:
        m = R.f32(mom)
        _close((1 - m) * d["rmean"].double() + m * f["mean"].detach(), bn.running_mean, "running_mean")
        _close((1 - m) * d["rvar"].double() + m * f["var"].detach() * B / (B - 1.0), bn.running_var, "running_var")
        assert float(f["var"].detach()[3]) == 0.0                                          # the constant column
    else:
        assert torch.equal(bn.running_mean, d["rmean"].double()) and torch.equal(f["mean"], d["rmean"].double())
    assert float(gam.detach()[1]) == 0.0 == float(bet.detach()[1]) and float(gg[0][:, 1].abs().max()) == 0.0 == float(gg[1][1])
    assert float(gam.detach()[2]) == 0.0 < float(bet.detach()[2]) and float(gg[0][:, 2].abs().max()) == 0.0 != float(gg[1][2])


def test_mlp_shapes_meet_the_edges_they_are_listed_for():
    """the shapes of test_gpu_decoder_kernels.py's mlp_head section: which kernel set each takes, the blocks of 64 rows and sum_parts'
    unroll of eight, and the workspace the library reports (stat / red: 2 H + 2 floats and the fast set's per-block partials)"""
    import test_gpu_decoder_kernels as DK
    lib = _library()
    cd = R.ceil_div
    assert DK.MLP_FAST == [(2, 1, 1), (63, 16, 16), (64, 16, 16), (65, 7, 12), (130, 12, 7), (513, 16, 1), (1024, 8, 8), (4099, 16, 16)]
    assert DK.MLP_GENERAL == [(5, 17, 3), (77, 24, 16), (256, 33, 17), (257, 8, 40), (300, 64, 64)] and DK.MLP_EVAL_ONLY == [(1, 16, 16)]
    assert all(R.mlp_fast(H, L) for _, H, L in DK.MLP_FAST + DK.MLP_EVAL_ONLY) and not any(R.mlp_fast(H, L) for _, H, L in DK.MLP_GENERAL)
    nblk = [cd(B, R.MLP_RB) for B, _, _ in DK.MLP_FAST]
    assert nblk == [1, 1, 1, 2, 3, 9, 16, 65] and [n % 8 for n in nblk] == [1, 1, 1, 2, 3, 1, 0, 1]
    assert any(L > H for _, H, L in DK.MLP_FAST) and any(H > L for _, H, L in DK.MLP_FAST)
    assert (257, 8, 40) in DK.MLP_GENERAL and 8 <= R.MLP_HP < 40                        # H <= 16 alone does not select the fast set
    assert {B for B, _, _ in DK.MLP_GENERAL} >= {5, 256, 257}                            # under, at and over one pass of a block's 256 threads
    for B, H, L in DK.MLP_FAST + DK.MLP_GENERAL + DK.MLP_EVAL_ONLY:
        part = cd(B, R.MLP_RB) * max(2 * 2 * R.MLP_HP, 3 * R.MLP_HP + R.MLP_HP * R.MLP_HP) if R.mlp_fast(H, L) else 0
        assert lib.coskad_mlp_head_ws_floats(B, H, L) == 2 * H + 2 + part, (B, H, L)


def _mlp_shapes():
    import test_gpu_decoder_kernels as DK
    return [(s, t) for s in DK.MLP_FAST + DK.MLP_GENERAL for t in (True, False)] + [(s, False) for s in DK.MLP_EVAL_ONLY]


@pytest.mark.parametrize("shape,training", _mlp_shapes())
def test_mlp_kink_share_of_the_reference_alone(shape, training):
    """the mlp_head test leaves out of dy the elements whose double y2 is non-zero and within the forward's and the backward's rounding
    bound of 0; from the reference alone their share is within the test's cap at every shape and mode it runs, every reference value
    and bound is finite, and the planted features are what the test says: an exact 0 is never a kink"""
    import test_gpu_decoder_kernels as DK
    B, H, L = shape
    c = DK.mlp_case(B, H, L, training)
    assert c["share"] <= DK.KINK_CAP, c["share"]
    assert all(np.isfinite(v).all() for v in c["ref"].values()) and all(np.isfinite(v).all() and (v >= 0).all() for v in c["bound"].values())
    if H >= R.MLP_PLANTS:
        assert not c["kink"][:, 1].any() and not c["kink"][:, 2].any()
        assert not c["ref"]["dy"][:, 1].any() and not c["ref"]["dy"][:, 2].any() and c["ref"]["dgamma"][2] != 0 and c["ref"]["dgamma"][1] == 0


@pytest.mark.parametrize("Co,TV,n", [(1, 1, 1), (3, 63, 37), (3, 257, 1), (32, 204, 37)])
def test_fold_case_bounds_are_finite_and_ordered(Co, TV, n):
    """fold_case on the host: every reference value finite, every bound finite and non-negative, the float64 outputs' bounds far below
    the float32 ones', and the all-zero branch's variance exactly 0"""
    import test_gpu_decoder_kernels as DK
    c = DK.fold_case(Co, TV, n)
    assert all(np.isfinite(v).all() for v in c["ref"].values()) and all(np.isfinite(v).all() and (v >= 0).all() for v in c["bound"].values())
    for q in ("xbar", "xx"):
        assert (c["bound"][q] <= 1e-9 * np.maximum(np.abs(c["ref"][q]).max(), 1.0)).all()
    if Co >= 2:
        assert float(c["var"][0, 1]) == 0.0
