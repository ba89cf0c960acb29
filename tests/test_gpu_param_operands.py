"""The one-clip-per-workgroup layer kernels with their parameter operands (bias quad, folded-weight columns, temporal records)
held in registers across the clip loop (csrc/fused_apply_next_bpc.hip, fused_apply_bpc.hip), and the fused backward
(csrc/fused_bwd.hip), against the split / recompute kernels of the same library at the batch sizes where a clip loop can go
wrong: one clip, fewer clips than waves would share, and grid + 3 (every workgroup takes one clip, three take a second one, and
the next-clip prefetch of all the others runs out of range).  Tolerances: test_apply_next_vs_separate_kernels (forward) and
test_fused_backward_ragged_batch_vs_split_kernels (backward).  Every kernel is run twice: the outputs must be bitwise equal."""
import numpy as np
import pytest
import torch

from test_gpu_backward import close, dev, make_layer_state
from test_gpu_forward import _bn_bufs, _rand_layer

pytestmark = pytest.mark.gpu

T, V, GUARD, POISON = 12, 17, 4096, 12345.0


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _untouched(buf, n, name):
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + n:] == POISON).all()), f"wrote outside {name}"


def _stats(x, L, Co, sl_in, ws):
    Z = torch.empty_like(x)
    b, zero = _bn_bufs(Co), torch.zeros(Co, device="cuda")
    wfold, bias, _ = ops().layer_train_stats(x, L["A"], L["T"], sl_in, L["Wt"], zero.clone(), L["gt"], L["bet"], b[0], b[1], b[2],
                                             L["Wr"], zero.clone(), L["gr"], L["ber"], b[3], b[4], b[5], ws, Z=Z)
    return Z, wfold, bias


def ops():
    from coskad_amd import ops as o
    return o


# (2, 32), (32, 16), (16, 32): k_layer_apply_next_bpc<0,2>, <2,1>, <1,2>; (16, 16): the wave-per-clip kernel (fused_apply_next.hip)
@pytest.mark.parametrize("B", [1, 5, 1027])
@pytest.mark.parametrize("Ci,Co,Cn", [(2, 32, 16), (32, 16, 32), (16, 32, 64), (16, 16, 16)])
def test_apply_next_param_operands_vs_separate_kernels(Ci, Co, Cn, B):
    o = ops()
    g = torch.Generator().manual_seed(Ci * 131 + Co * 7 + Cn + B)
    x = torch.randn(B, Ci, T, V, generator=g).cuda()
    L1, L2 = _rand_layer(g, Ci, Co), _rand_layer(g, Co, Cn)
    sl_in = torch.tensor([0.2], device="cuda") if Ci > 2 else None
    ws = torch.empty(o.train_stats_ws_bytes(64), dtype=torch.uint8, device="cuda")
    Z, wfold, bias = _stats(x, L1, Co, sl_in, ws)
    # separate kernels: apply, then the next layer's statistics pass over U
    U_ref = o.layer_apply_z(Z, x, L1["A"], L1["T"], wfold, bias, Co, in_slope=sl_in)
    zero2 = torch.zeros(Cn, device="cuda")
    Z2_ref = torch.empty_like(U_ref)
    br = _bn_bufs(Cn)
    ref = o.layer_train_stats(U_ref, L2["A"], L2["T"], L1["slope"], L2["Wt"], zero2.clone(), L2["gt"], L2["bet"], br[0], br[1], br[2],
                              L2["Wr"], zero2.clone(), L2["gr"], L2["ber"], br[3], br[4], br[5], ws, Z=Z2_ref)
    ftab = torch.empty(o.ftab_floats(), device="cuda")
    o.build_ftabs([L2["A"]], [L2["T"]], [ftab])
    rows_max = o.layer_apply_next_rows(B, Ci, Co)
    E = 2 * (Co * Co + Co)
    n = B * Co * T * V
    runs = []
    for _ in range(2):
        bufU, U = _guarded((B, Co, T, V))
        bufZ, Z2 = _guarded((B, Co, T, V))
        bufP, partials = _guarded((rows_max * E,))
        _, _, rows = o.layer_apply_next(Z, x, wfold, bias, Co, sl_in, L1["slope"], ftab, partials, T, V, out=U, Z_next=Z2)
        torch.cuda.synchronize()
        for name, b, m in (("U", bufU, n), ("Z", bufZ, n), ("partials", bufP, rows_max * E)):
            _untouched(b, m, name)
        assert rows == rows_max
        runs.append((U, Z2, partials))
    for name, a, b in zip(("U", "Z_next", "partials"), runs[0], runs[1]):
        assert torch.equal(a, b), f"{name}: two calls differ"
    U, Z2, partials = runs[0]
    bf = _bn_bufs(Cn)
    got = o.layer_train_fold(partials, rows_max, B, T, V, L2["Wt"], zero2.clone(), L2["gt"], L2["bet"], bf[0], bf[1], bf[2],
                             L2["Wr"], zero2.clone(), L2["gr"], L2["ber"], bf[3], bf[4], bf[5], ws)
    np.testing.assert_allclose(U.cpu().numpy(), U_ref.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(Z2.cpu().numpy(), Z2_ref.cpu().numpy(), rtol=1e-4, atol=2e-5)
    for name, a, r in zip(("wfold", "bias", "stat"), got, ref):
        np.testing.assert_allclose(a.cpu().numpy(), r.cpu().numpy(), rtol=2e-4, atol=2e-5, err_msg=name)
    for i, (a, r) in enumerate(zip(bf, br)):
        np.testing.assert_allclose(a.cpu().numpy(), r.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=f"bn buffer {i}")


# (32, 64): k_layer_apply_bpc<2> (768 workgroups); the other pairs: the K-ring kernels of fused_apply.hip
@pytest.mark.parametrize("B", [1, 5, 771])
@pytest.mark.parametrize("Ci,Co", [(32, 64), (16, 32), (32, 16), (16, 16)])
def test_apply_param_operands_vs_recompute_kernel(Ci, Co, B):
    o = ops()
    g = torch.Generator().manual_seed(Ci * 7 + Co + B)
    x = torch.randn(B, Ci, T, V, generator=g).cuda()
    L = _rand_layer(g, Ci, Co)
    sl = torch.tensor([0.2], device="cuda")
    ws = torch.empty(o.train_stats_ws_bytes(Ci), dtype=torch.uint8, device="cuda")
    Z, wfold, bias = _stats(x, L, Co, sl, ws)
    outs = []
    for _ in range(2):
        buf, out = _guarded((B, Co, T, V))
        o.layer_apply_z(Z, x, L["A"], L["T"], wfold, bias, Co, in_slope=sl, out=out)
        torch.cuda.synchronize()
        _untouched(buf, out.numel(), "the output")
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    ref = o.layer_apply(x, L["A"], L["T"], wfold, bias, Co, in_slope=sl)
    err = (outs[0] - ref).abs().max().item()
    print(f"apply ({Ci}, {Co}) B = {B}: max |stored-Z - recompute| = {err:.3e}")
    np.testing.assert_allclose(outs[0].cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-5)


# the four layers of the default stack on k_layer_bwd_bpc (two workgroups per CU: 512) and (16, 16) on the three-per-CU instantiation
@pytest.mark.parametrize("B", [1, 5, 515])
@pytest.mark.parametrize("Ci,Co", [(2, 32), (32, 16), (16, 32), (32, 64), (16, 16)])
def test_fused_backward_param_operands_vs_split_kernels(Ci, Co, B):
    o = ops()
    first = Ci == 2
    st = make_layer_state(Ci, Co, V, seed=Ci + Co)
    g = torch.Generator().manual_seed(B)
    x_pre = dev(torch.randn(B, Ci, T, V, generator=g))
    probe = dev(torch.randn(B, Co, T, V, generator=g) * 0.1)
    d = {k[2:]: dev(v) for k, v in st.items()}
    sl = None if first else dev(torch.tensor([0.2]))
    Wt, Wr = d["tcn.0.weight"].reshape(Co, Ci), d["residual.0.weight"].reshape(Co, Ci)
    ws = torch.empty(max(o.train_stats_ws_bytes(Ci), o.layer_bwd_ws_bytes(B, Ci, Co, T, V)), dtype=torch.uint8, device="cuda")
    Z = torch.empty_like(x_pre)
    _, _, stat = o.layer_train_stats(
        x_pre, d["gcn.A"], d["gcn.T"], sl, Wt, d["tcn.0.bias"], d["tcn.1.weight"], d["tcn.1.bias"],
        d["tcn.1.running_mean"], d["tcn.1.running_var"], d["tcn.1.num_batches_tracked"],
        Wr, d["residual.0.bias"], d["residual.1.weight"], d["residual.1.bias"],
        d["residual.1.running_mean"], d["residual.1.running_var"], d["residual.1.num_batches_tracked"], ws, Z=Z)

    def run(zz):
        z = lambda *s_: torch.full(s_, float("nan"), device="cuda")
        gr = {"A": z(T, V, V), "T": z(V, T, T), "Wt": z(Co, Ci), "bt": z(Co), "gt": z(Co), "bet": z(Co), "Wr": z(Co, Ci),
              "br": z(Co), "gr": z(Co), "ber": z(Co)}
        if not first:
            gr["slope_in"] = z(1)
        buf, dIn = _guarded(tuple(x_pre.shape))
        o.layer_bwd(x_pre, probe, d["gcn.A"], d["gcn.T"], sl, stat, Wt, d["tcn.1.weight"], Wr, d["residual.1.weight"], gr, ws,
                    need_dx=not first, dIn=dIn if not first else None, Z=zz)
        torch.cuda.synchronize()
        _untouched(buf, x_pre.numel(), "dIn")
        return dIn, gr

    dIn_f, g_f = run(Z)
    dIn_2, g_2 = run(Z)
    dIn_s, g_s = run(None)
    if not first:
        assert torch.equal(dIn_f, dIn_2), "dIn: two calls differ"
        close(dIn_f, dIn_s.cpu(), rtol=5e-4, atol_rel=5e-5, msg="dIn")
    for k in g_s:
        assert torch.equal(g_f[k], g_2[k]), f"{k}: two calls differ"
        a, b = g_f[k].cpu().numpy(), g_s[k].cpu().numpy()
        assert np.isfinite(a).all(), k
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4 * max(np.abs(b).max(), 1e-9), err_msg=k)
