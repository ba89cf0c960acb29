"""The fused layer backward (csrc/fused_bwd.hip) with its LDS operand reads issued as batches a step ahead of their MFMAs (dT /
Kr.X steps, the chain loops, the K pass) and, at 32 -> 64 with the chain, its dT and chain sums parked in LDS outside their
phases -- with the chain on (the data kernel also forms the batch reductions of the layer below) against the split kernels of
the same library.  Batch sizes: one clip, fewer clips than waves, 512 + 3 (three workgroups take a second clip: a parked sum is
restored, added to and parked again) and 2 x 512 + 3 (a third clip); the pipelines' first and last steps run at every size.
(16, 16, 16) has no chain kernel: its data kernel (three workgroups per CU, one operand set) runs without the chain.
Tolerances of the upper layer: test_gpu_param_operands.test_fused_backward_param_operands_vs_split_kernels; of the lower layer,
which receives the chain's sums: test_gpu_backward.test_backward_chain_below_stats_vs_own_pass (same quantity, same reference).
Every kernel is run twice: the outputs must be bitwise equal."""
import numpy as np
import pytest
import torch

from test_gpu_backward import close, dev, make_layer_state

pytestmark = pytest.mark.gpu

T, V, GUARD, POISON = 12, 17, 4096, 12345.0


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), POISON, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _untouched(buf, n, name):
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + n:] == POISON).all()), f"wrote outside {name}"


def _grads(Ci, Co, slope):
    z = lambda *s_: torch.full(s_, float("nan"), device="cuda")
    gr = {"A": z(T, V, V), "T": z(V, T, T), "Wt": z(Co, Ci), "bt": z(Co), "gt": z(Co), "bet": z(Co), "Wr": z(Co, Ci),
          "br": z(Co), "gr": z(Co), "ber": z(Co)}
    if slope:
        gr["slope_in"] = z(1)
    return gr


@pytest.mark.parametrize("B", [1, 5, 515, 1027])
@pytest.mark.parametrize("C0,C1,C2", [(16, 32, 64), (32, 16, 32), (2, 32, 16), (16, 16, 16)])
def test_fused_backward_operand_batches_with_chain_vs_split_kernels(C0, C1, C2, B):
    from coskad_amd import ops
    st1, st2 = make_layer_state(C0, C1, V, seed=C0 + C1), make_layer_state(C1, C2, V, seed=C1 + C2 + 1)
    g = torch.Generator().manual_seed(B * 7 + C0)
    x = dev(torch.randn(B, C0, T, V, generator=g))
    probe = dev(torch.randn(B, C2, T, V, generator=g) * 0.1)
    d1, d2 = {k[2:]: dev(v) for k, v in st1.items()}, {k[2:]: dev(v) for k, v in st2.items()}
    sl0 = dev(torch.tensor([0.3])) if C0 > 2 else None
    sl = dev(torch.tensor([0.2]))
    ws = torch.empty(max(ops.train_stats_ws_bytes(C1), ops.train_stats_ws_bytes(C0), ops.layer_bwd_ws_bytes(B, C1, C2, T, V),
                         ops.layer_bwd_ws_bytes(B, C0, C1, T, V)), dtype=torch.uint8, device="cuda")

    def stats(xin, dd, Ci, Co, slope):
        Z = torch.empty(B, Ci, T, V, device="cuda")
        wf, bi, stat = ops.layer_train_stats(
            xin, dd["gcn.A"], dd["gcn.T"], slope, dd["tcn.0.weight"].reshape(Co, Ci), dd["tcn.0.bias"], dd["tcn.1.weight"], dd["tcn.1.bias"],
            dd["tcn.1.running_mean"], dd["tcn.1.running_var"], dd["tcn.1.num_batches_tracked"],
            dd["residual.0.weight"].reshape(Co, Ci), dd["residual.0.bias"], dd["residual.1.weight"], dd["residual.1.bias"],
            dd["residual.1.running_mean"], dd["residual.1.running_var"], dd["residual.1.num_batches_tracked"], ws, Z=Z)
        return Z, wf, bi, stat
    Z1, wf1, b1, stat1 = stats(x, d1, C0, C1, sl0)
    U1 = ops.layer_apply_z(Z1, x, d1["gcn.A"], d1["gcn.T"], wf1, b1, C1, in_slope=sl0)
    Z2, _, _, stat2 = stats(U1, d2, C1, C2, sl)
    rows = ops.layer_bwd_below_rows(B, C1, C2, C0, T, V)
    assert (rows > 0) == ((C0, C1, C2) != (16, 16, 16))
    nb = ops.layer_bwd_below_floats(B, C1, C2, C0, T, V) if rows else 0

    def upper(zz, chain):
        g2 = _grads(C1, C2, True)
        bufI, dI = _guarded(U1.numel())
        bufS, bs = _guarded(nb) if chain else (None, None)
        ops.layer_bwd(U1, probe, d2["gcn.A"], d2["gcn.T"], sl, stat2, d2["tcn.0.weight"].reshape(C2, C1), d2["tcn.1.weight"],
                      d2["residual.0.weight"].reshape(C2, C1), d2["residual.1.weight"], g2, ws, dIn=dI.view_as(U1), Z=zz,
                      below=(x, Z1, sl0, bs) if chain else None)
        torch.cuda.synchronize()
        _untouched(bufI, U1.numel(), "dIn")
        if chain:
            _untouched(bufS, nb, "below_stats")
        return dI.view_as(U1), g2, bs

    def lower(dU1, stats_in):
        g1 = _grads(C0, C1, sl0 is not None)
        dX = ops.layer_bwd(x, dU1, d1["gcn.A"], d1["gcn.T"], sl0, stat1, d1["tcn.0.weight"].reshape(C1, C0), d1["tcn.1.weight"],
                           d1["residual.0.weight"].reshape(C1, C0), d1["residual.1.weight"], g1, ws, need_dx=sl0 is not None, Z=Z1,
                           stats_in=stats_in)
        torch.cuda.synchronize()
        return dX, g1

    chain = rows > 0
    dU_f, g2_f, bs_f = upper(Z2, chain)
    dU_2, g2_2, bs_2 = upper(Z2, chain)
    dU_s, g2_s, _ = upper(None, False)
    assert torch.equal(dU_f, dU_2), "dIn: two calls differ"
    if chain:
        # (bit patterns: the buffer ends in fp64 sums, whose halves read as floats may be NaNs)
        assert torch.equal(bs_f.view(torch.int32), bs_2.view(torch.int32)), "below_stats: two calls differ"
    close(dU_f, dU_s.cpu(), rtol=5e-4, atol_rel=5e-5, msg="dIn")
    for k in g2_s:
        assert torch.equal(g2_f[k], g2_2[k]), f"{k}: two calls differ"
        a, b = g2_f[k].cpu().numpy(), g2_s[k].cpu().numpy()
        assert np.isfinite(a).all(), k
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4 * max(np.abs(b).max(), 1e-9), err_msg=k)
    if not chain:
        return
    # the sums the chain formed, through the lower layer's backward, against that layer's own statistics pass on the same dU
    dX_c, g1_c = lower(dU_f, (bs_f, rows))
    dX_o, g1_o = lower(dU_f, None)
    if dX_o is not None:
        close(dX_c, dX_o.cpu(), rtol=1e-3, atol_rel=1e-4, msg="dX of the lower layer")
    gmax = max(float(v.abs().max()) for v in g1_o.values())
    for k in g1_o:
        a, b = g1_c[k].cpu().numpy(), g1_o[k].cpu().numpy()
        assert np.isfinite(a).all(), k
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4 * max(np.abs(b).max(), 1e-9) + 2e-5 * gmax, err_msg="lower layer " + k)
