"""The autoencoder and the spherical VAE on the flat train step at the window lengths 8 / 16 / 24: the few-channel
(4 -> 2) layer on the stored-Z layer kernels (csrc/train_window_moments.hip with four input channels, csrc/first_layer.hip's apply and
stage 1, csrc/train_window_flat.hip's data pass with M = 4 / K = 6, csrc/gcn_window.hip's parameter kernel), the `narrow` segment of
trainer._FlatStack(window=True), STSAETrainStep(fused_window=True), the wrappers and the command line.

Tolerances are the project's own: the statistics pass as tests/test_gpu_train_window.py::test_statistics_pass, a layer's outputs
rtol = atol = 1e-4, gradients by that file's _check_grads, running statistics by its _check_running; the model steps as
tests/test_gpu_ae_step.py states them for 12 frames.

Batch sizes of the layer test: a 16-row tile of the statistics pass holds four clips of four channels and a workgroup pass 2 or 4 such
tiles (8 or 16 clips) -- B = 1 is one clip in a tile, B = 5 a ragged second tile, B = 17 a ragged second pass."""
import ast
import glob
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

from oracle import ref_cpu as R
from test_gpu_train_window import GUARD, SENTINEL, _check_grads, _check_running, _guards_untouched, _inside, _layer_state, _stream, _tables

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(T, V) for T in (8, 16, 24) for V in (17, 25)]
NAMES = {"A": "L.gcn.A", "T": "L.gcn.T", "Wt": "L.tcn.0.weight", "bt": "L.tcn.0.bias", "gt": "L.tcn.1.weight", "bet": "L.tcn.1.bias",
         "Wr": "L.residual.0.weight", "br": "L.residual.0.bias", "gr": "L.residual.1.weight", "ber": "L.residual.1.bias"}


# ---- 1. the few-channel layer through the ABI ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_slope", [False, True])
@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("T,V", GEOMETRIES)
def test_few_channel_statistics_pass(T, V, B, with_slope):
    """coskad_layer_train_moments_f32 with four input channels: Z and the fp64 moment sums against fp64 arithmetic"""
    from coskad_amd import _lib, ops
    Ci = 4
    g = torch.Generator().manual_seed(T * 1000 + V * 10 + Ci + B)
    x = torch.randn(B, Ci, T, V, generator=g)
    A, Tm = _tables(T, V, g)
    slope = torch.full((1,), 0.3) if with_slope else None
    xa = R.prelu(x, slope) if with_slope else x
    z_ref = R.gcn(xa, A, Tm)
    xd64, zd64 = xa.double().transpose(0, 1).reshape(Ci, -1), R.gcn(xa.double(), A.double(), Tm.double()).transpose(0, 1).reshape(Ci, -1)
    want = [xd64 @ xd64.t(), xd64.sum(1), zd64 @ zd64.t(), zd64.sum(1)]
    nan = float("nan")
    (xd, xp), (Ad, Ap), (Td, Tp) = _inside(x, nan), _inside(A, nan, 37), _inside(Tm, nan, 37)
    ws = torch.empty(ops.train_stats_ws_bytes(Ci), dtype=torch.uint8, device="cuda")
    sd = slope.cuda() if with_slope else None

    def run():
        Z, Zp = _inside(torch.full(x.shape, SENTINEL), SENTINEL)
        sums, sp = _inside(torch.full((2 * (Ci * Ci + Ci),), SENTINEL, dtype=torch.float64), SENTINEL, 4)
        _lib.call("coskad_layer_train_moments_f32", xd, Ad, Td, sd, Z, sums, ws, ws.numel(), B, Ci, T, V, _stream())
        _guards_untouched(Zp, SENTINEL, "Z")
        _guards_untouched(sp, SENTINEL, "sums", 4)
        return Z.clone(), sums.clone()

    Z, sums = run()
    Z2, sums2 = run()
    assert torch.equal(Z, Z2) and torch.equal(sums, sums2), "two calls differ"
    for p, n, gd in ((xp, "in", GUARD), (Ap, "A", 37), (Tp, "T", 37)):
        _guards_untouched(p, nan, n, gd)
    assert torch.isfinite(Z).all() and torch.isfinite(sums).all()
    np.testing.assert_allclose(Z.cpu().numpy(), z_ref.numpy(), rtol=1e-5, atol=1e-5)
    s = sums.cpu()
    blocks = [s[:Ci * Ci].view(Ci, Ci), s[Ci * Ci:Ci * Ci + Ci], s[Ci * Ci + Ci:2 * Ci * Ci + Ci].view(Ci, Ci), s[2 * Ci * Ci + Ci:]]
    for got, w, n in zip(blocks, want, ("sum x x^T", "sum x", "sum z z^T", "sum z")):
        np.testing.assert_allclose(got.numpy(), w.numpy(), rtol=0, atol=1e-5 * float(w.abs().max()), err_msg=n)


@pytest.mark.parametrize("with_slope", [False, True])
@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("T,V", GEOMETRIES)
def test_few_channel_layer_forward_backward(T, V, B, with_slope):
    """statistics pass + fold, apply and backward of a (4 -> 2) layer with a convolution residual, every output inside guard bands:
    U, every parameter gradient, dIn, the producer's slope gradient and the running statistics against the oracle's fp64 autograd;
    twice bit for bit; once more accumulating into pre-filled destinations"""
    from coskad_amd import engine, ops
    from coskad_amd.models.graph_layers.stsgcn import ST_GCNN_layer, layer_tensors
    Ci, Co = 4, 2
    assert ops.layer_train_window_narrow_ok(T, V, Ci, Co) and not ops.layer_train_window_ok(T, V, Ci, Co)
    st = _layer_state(Ci, Co, T, V, seed=Ci * 100 + Co + T + V, identity=False)
    g = torch.Generator().manual_seed(7 + B)
    x = torch.randn(B, Ci, T, V, generator=g)                    # activated input, or the producer's pre-activation
    probe = torch.randn(B, Co, T, V, generator=g) / (B * T * V) ** 0.5
    in_slope = torch.full((1,), 0.2) if with_slope else None
    pk = [k for k in st if R.is_param_key(k) and st[k].is_floating_point() and k != "L.prelu.weight"]
    stc = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in st.items()}
    for k in pk:
        stc[k].requires_grad_(True)
    xo = x.double().requires_grad_(True)
    so = in_slope.double().requires_grad_(True) if with_slope else None
    u_ref = R.st_gcnn_layer(R.prelu(xo, so) if with_slope else xo, stc, "L", training=True, return_preact=True)
    (u_ref * probe.double()).sum().backward()
    want = {k: stc[k].grad.float() for k in pk}
    if with_slope:
        want["slope_in"] = so.grad.float()
    nan = float("nan")

    def run(accumulate):
        layer = ST_GCNN_layer(Ci, Co, (1, 1), 1, T, V, 0.0)
        layer.load_state_dict({k[2:]: v for k, v in st.items()}, strict=True)
        layer.cuda().train()
        L = layer_tensors(layer)
        (xd, xp), (pd, pp) = _inside(x, nan), _inside(probe, nan)
        sd = in_slope.cuda() if with_slope else None
        buf = torch.empty(ops.train_stats_ws_bytes(Ci), dtype=torch.uint8, device="cuda")
        (Z, Zp), (U, Up), (dIn, dp) = (_inside(torch.full(s, SENTINEL), SENTINEL) for s in (x.shape, probe.shape, x.shape))
        wfold, bias, stat = ops.layer_train_stats(xd, L.A, L.T, sd, L.w2(L.Wt), L.bt, L.gt, L.bet, L.rm_t, L.rv_t, L.nbt_t,
                                                  L.w2(L.Wr), L.br, L.gr, L.ber, L.rm_r, L.rv_r, L.nbt_r, buf, momentum=L.step_momentum(), Z=Z)
        ops.layer_apply_z(Z, xd, L.A, L.T, wfold, bias, Co, in_slope=sd, out=U)
        gg = torch.Generator().manual_seed(11)
        base, dst, parents = {}, {}, {}
        for k, n in list(NAMES.items()) + ([("slope_in", "slope_in")] if with_slope else []):
            shape = (1,) if n == "slope_in" else st[n].shape
            b0 = torch.randn(shape, generator=gg) if accumulate else torch.full(shape, SENTINEL)
            dst[k], parents[k] = _inside(b0, SENTINEL, 37)
            base[n] = b0
        wsb = torch.empty(ops.layer_bwd_ws_bytes(B, Ci, Co, T, V), dtype=torch.uint8, device="cuda")
        ops.layer_bwd(xd, pd, L.A, L.T, sd, stat, L.w2(L.Wt), L.gt, L.w2(L.Wr), L.gr, engine._as2d(dst), wsb, need_dx=True, dIn=dIn,
                      accumulate=accumulate, Z=Z)
        torch.cuda.synchronize()
        for p, n in ((Zp, "Z"), (Up, "U"), (dp, "dIn")):
            _guards_untouched(p, SENTINEL, n)
        for p, n in ((xp, "in"), (pp, "dU")):
            _guards_untouched(p, nan, n)
        for k, p in parents.items():
            _guards_untouched(p, SENTINEL, "grad " + k, 37)
        got = {n: dst[k].clone() for k, n in list(NAMES.items()) + [("slope_in", "slope_in")] if k in dst}
        return layer, U.clone(), got, base, dIn.clone()

    layer, u, got, _, dIn = run(False)
    np.testing.assert_allclose(u.cpu().numpy(), u_ref.detach().float().numpy(), rtol=1e-4, atol=1e-4)
    assert _check_grads(got, want) == len(want) - 2
    stf = {k: (v.float() if v.is_floating_point() else v) for k, v in stc.items()}
    assert _check_running({"L." + k: v for k, v in layer.state_dict().items()}, {k: v.detach() for k, v in stf.items()}) == 4
    b = xo.grad.float().numpy()
    np.testing.assert_allclose(dIn.cpu().numpy(), b, rtol=5e-4, atol=5e-5 * float(np.abs(b).max()))
    _, u1, got1, _, dIn1 = run(False)
    assert torch.equal(u, u1) and torch.equal(dIn, dIn1) and all(torch.equal(got[k], got1[k]) for k in got), "two calls differ"
    _, u2, got2, base2, dIn2 = run(True)
    assert torch.equal(u, u2) and torch.equal(dIn, dIn2)
    assert _check_grads(got2, want, {n: base2[n] for n in want}) == len(want) - 2


# ---- 2. the narrow segment against the composed layer ----------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V", [(8, 17), (16, 25)])
def test_narrow_segment_equals_the_composed_layer(T, V):
    """a (32 -> 2) layer as trainer._NarrowLayer under window=True (convolutions first, then the virtual (4 -> 2) layer on the window
    kernels) against the same layer as trainer._WideLayer (stsgcn.wide_forward / wide_backward), both fed one pre-activation and slope"""
    from coskad_amd import engine, ops, trainer
    from coskad_amd.models.graph_layers.stsgcn import ST_GCNN_layer
    Ci, Co, B = 32, 2, 5
    st = _layer_state(Ci, Co, T, V, seed=T + V, identity=False)
    g = torch.Generator().manual_seed(3)
    h = torch.randn(B, Ci, T, V, generator=g).cuda()
    d = (torch.randn(B, Co, T, V, generator=g) / (B * T * V) ** 0.5).cuda()
    slope = torch.full((1,), 0.2).cuda()
    res = {}
    for kind in ("narrow", "wide"):
        layer = ST_GCNN_layer(Ci, Co, (1, 1), 1, T, V, 0.0)
        layer.load_state_dict({k[2:]: v for k, v in st.items()}, strict=True)
        seq = torch.nn.Sequential(layer).cuda().train()
        fp = trainer.FlatParams(seq)
        stack = trainer._FlatStack([layer], fp, "", window=(kind == "narrow"))
        assert [s.kind for s in stack.segs] == [kind]
        seg, ws = stack.segs[0], engine.Workspace()
        dslope_in = torch.full((1,), SENTINEL, device="cuda")
        u, out_slope, saved = seg.forward(h, slope, ws)
        if kind == "narrow":
            assert type(seg) is trainer._NarrowLayer and (seg.virt.Ci, seg.virt.Co) == (4, 2)
            out = ops.prelu_fwd(u, out_slope)
            dU = ops.prelu_bwd(u, d, out_slope, seg.out_slope_grad)
        else:
            assert out_slope is None
            out, dU = u, d
        dIn = seg.backward(saved, dU, ws, True, dslope_in)
        torch.cuda.synchronize()
        grads = {"L." + n[2:]: v.detach().cpu().clone() for n, v in fp.gviews.items()}
        grads["slope_in"] = dslope_in.cpu()
        res[kind] = (out.cpu(), dIn.cpu(), grads, {"L." + k: v.cpu() for k, v in layer.state_dict().items()})
    a, b = res["wide"], res["narrow"]
    np.testing.assert_allclose(b[0].numpy(), a[0].numpy(), rtol=1e-4, atol=1e-4)
    r = a[1].numpy()
    np.testing.assert_allclose(b[1].numpy(), r, rtol=5e-4, atol=5e-5 * float(np.abs(r).max()))
    assert set(a[2]) == set(b[2]) and "L.prelu.weight" in a[2]
    assert _check_grads(b[2], a[2]) == len(a[2]) - 2
    assert _check_running(b[3], a[3]) == 4


# ---- 3. the autoencoder step against the CPU oracle --------------------------------------------------------------------------------------

def _ae_state(T, V, latent=16):
    st = R.init_stse_state(T=T, V=V, latent=latent, seed=7, decoder=True)
    st["c"] = torch.linspace(-0.1, 0.1, latent)
    return st


def _ae_model(st, T, V, latent=16):
    from coskad_amd.models.sts.ae import STSAE
    m = STSAE(2, [32, 16, 32], 64, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    return m


def _kinds(stack):
    return [s.kind for s in stack.segs]


@pytest.mark.parametrize("T,V,B", [(8, 17, 6), (16, 25, 5), (24, 17, 3), (24, 25, 2), (8, 17, 37), (8, 25, 11)])
def test_window_autoencoder_step_vs_oracle(T, V, B):
    """default widths, latent 16: losses, every gradient, the running statistics and (lr = 0) the untouched parameters of one
    STSAETrainStep(fused_window=True) step against the CPU oracle's autograd; tolerances of
    tests/test_gpu_ae_step.py::test_flat_autoencoder_step_default_widths_vs_oracle.  (For these seeds the fp32 oracle differs from the
    same oracle in fp64 by at most 0.5 % of the gradient tolerance.)"""
    from coskad_amd.trainer import STSAETrainStep
    st = _ae_state(T, V)
    x = R.synthetic_clips(B, 2, T, V, seed=8)
    m = _ae_model(st, T, V)
    eng = STSAETrainStep(m.cuda().train(), mode='ae', lr=0.0, alpha=0.0, lambda_=0.3, fused_window=True)
    assert _kinds(eng.enc) == ['window'] and _kinds(eng.dec) == ['window', 'narrow'] and eng.lowrank is not None
    out = eng.step(x.cuda())
    torch.cuda.synchronize()
    params = {k: v.clone().requires_grad_(True) for k, v in st.items() if R.is_param_key(k) and v.is_floating_point()}
    so = {k: v.clone() for k, v in st.items()}
    so.update(params)
    z = R.stse_encode(x, so, training=True)
    xr = R.stsae_decode(z, so, 64, T, V, training=True)
    l_rec, l_h = ((xr - x) ** 2).mean(), R.mse_to_center(z, st["c"])
    (0.3 * l_rec + l_h).backward()
    print("rec", float(out['rec']), float(l_rec.detach()), "head", float(out['head']), float(l_h.detach()))
    np.testing.assert_allclose(float(out['rec']), float(l_rec.detach()), rtol=1e-4)
    np.testing.assert_allclose(float(out['head']), float(l_h.detach()), rtol=1e-4)
    assert set(params) == set(eng.fp.gviews)
    gmax = max(float(p.grad.abs().max()) for p in params.values())
    worst = (0.0, None)
    for n, p in params.items():
        r, a = p.grad.numpy(), eng.fp.gviews[n].cpu().numpy()
        use = float(np.max(np.abs(a - r) / (2e-3 * np.abs(r) + 2e-4 * np.abs(r).max() + 5e-5 * gmax)))
        worst = max(worst, (use, n))
    print("largest share of the gradient tolerance:", worst)
    for n, p in params.items():
        r = p.grad.numpy()
        np.testing.assert_allclose(eng.fp.gviews[n].cpu().numpy(), r, rtol=2e-3, atol=2e-4 * np.abs(r).max() + 5e-5 * gmax, err_msg=n)
    sd = m.state_dict()
    n_run = 0
    for k, v in so.items():
        if "running" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
            n_run += 1
    assert n_run == 32                                    # 8 layers x 2 BatchNorms x (mean, var): every layer has a conv residual
    for n in params:                                      # lr = 0: the fused Adam left every parameter where it was
        assert torch.equal(sd[n].cpu(), st[n]), n


# ---- 4. the same step on two routes ------------------------------------------------------------------------------------------------------

def test_window_autoencoder_step_equals_torch_adam_on_the_module_surface():
    """two steps with lr > 0 and alpha > 0 at (8, 17), B = 37: the flat step with fused_window and the module-surface path (autograd over
    the composed layers + calc_reg_loss in the loss + torch.optim.Adam) end with the same parameters; tolerances and the exclusion of
    the analytically-zero conv biases as in test_flat_autoencoder_step_equals_torch_adam_on_the_module_surface"""
    from coskad_amd.trainer import STSAETrainStep
    T, V = 8, 17
    st = _ae_state(T, V)
    x = R.synthetic_clips(37, 2, T, V, seed=8).cuda()
    res = []
    for flat in (True, False):
        m = _ae_model(st, T, V).cuda().train()
        if flat:
            eng = STSAETrainStep(m, mode='ae', lr=1e-3, alpha=1e-3, lambda_=0.5, fused_window=True)
            assert 'wide' not in _kinds(eng.enc) + _kinds(eng.dec)
            for _ in range(2):
                eng.step(x)
        else:
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)
            for _ in range(2):
                opt.zero_grad(set_to_none=True)
                z, xr = m(x)
                ps = [p for n, p in m.named_parameters() if 'bias' not in n]
                reg = 0.5 * sum((p ** 2).sum() for p in ps) / len(ps)
                (0.5 * ((xr - x) ** 2).mean() + ((z - m.c) ** 2).mean() + 1e-3 * reg).backward()
                opt.step()
        torch.cuda.synchronize()
        res.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    for k in res[0]:
        if k.endswith(("tcn.0.bias", "residual.0.bias")):
            continue        # analytically-zero gradients: autograd's rounding noise random-walks them under Adam
        np.testing.assert_allclose(res[0][k].numpy(), res[1][k].numpy(), rtol=2e-3, atol=3e-4, err_msg=k)


# ---- 5. the spherical VAE step -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V", [(8, 17), (16, 25)])
def test_window_vae_step_matches_module_autograd(T, V):
    """tests/test_gpu_ae_step.py::test_flat_vae_step_matches_module_autograd at a window length with fused_window: same torch seed,
    same PowerSpherical sample; losses and every gradient agree at that test's tolerances"""
    from coskad_amd.models.sts.vae import STSVAE, kl_ps_uniform
    from coskad_amd.trainer import STSAETrainStep
    make = lambda: STSVAE(2, [32, 16, 32], 64, 8, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0, distribution='ps')
    torch.manual_seed(3)
    st = {k: v.detach().clone() for k, v in make().state_dict().items()}
    x = R.synthetic_clips(24, 2, T, V, seed=4).cuda()
    phi, beta, gamma = 0.7, 0.3, 0.2
    m1 = make()
    m1.load_state_dict(st)
    m1.cuda().train()
    torch.manual_seed(11)
    z, xr, (q, p, kappa) = m1(x)
    l_rec, l_kl, l_exp = ((xr - x) ** 2).mean(), kl_ps_uniform(q, p).mean(), (1 / kappa).mean()
    (phi * l_rec + beta * l_kl + gamma * l_exp).backward()
    m2 = make()
    m2.load_state_dict(st)
    m2.cuda().train()
    eng = STSAETrainStep(m2, mode='vae', lr=0.0, alpha=0.0, phi=phi, beta=beta, gamma=gamma, fused_window=True)
    assert _kinds(eng.enc) == ['window'] and _kinds(eng.dec) == ['window', 'narrow'] and eng.lowrank is not None
    torch.manual_seed(11)
    out = eng.step(x)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out['z'].cpu().numpy(), z.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(out['rec']), float(l_rec), rtol=1e-4)
    np.testing.assert_allclose(float(out['head']), float(l_kl), rtol=1e-4)
    np.testing.assert_allclose(float(out['exp']), float(l_exp), rtol=1e-4)
    grads = {n: p.grad for n, p in m1.named_parameters()}
    gmax = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for n, ref in grads.items():
        if ref is None:
            continue
        r = ref.cpu().numpy()
        np.testing.assert_allclose(eng.fp.gviews[n].cpu().numpy(), r, rtol=2e-3, atol=2e-4 * np.abs(r).max() + 5e-5 * gmax, err_msg=n)


# ---- 6. the wrappers -----------------------------------------------------------------------------------------------------------------------

def _args(name, T, **over):
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", name)), Loader=yaml.FullLoader)
    cfg.update(dict(dict(create_experiment_dir=False, dataset_seg_len=T), **over))
    args, *_ = init_sub_args(Namespace(**cfg))
    return args, cfg


def test_autoencoder_wrapper_takes_the_flat_step_at_a_window_length():
    from coskad_amd.lit import LitAutoEncoder
    from coskad_amd.trainer import STSAETrainStep
    _, cfg = _args("euclidean_autoencoder_seg16.yaml", 16)
    assert cfg["dataset_seg_len"] == 16 and cfg["channels"] == [32, 16, 32] and cfg["h_dim"] == 64 and cfg["latent_dim"] == 16
    assert "fused_window" not in cfg and cfg["dir_name"].endswith("_seg16")
    x = R.synthetic_clips(64, 2, 16, 17, seed=5)
    batch = [x, None, None, None]
    logged = {}
    for fused in (None, False):
        args, _ = _args("euclidean_autoencoder_seg16.yaml", 16, **({} if fused is None else {"fused_window": fused}))
        torch.manual_seed(0)
        lit = LitAutoEncoder(args).cuda()
        lit.model.train()
        lit._make_optimiser('ae', lambda_=lit.lambda_)
        if fused is None:
            assert type(lit._flat) is STSAETrainStep
            assert 'wide' not in _kinds(lit._flat.enc) + _kinds(lit._flat.dec) and _kinds(lit._flat.dec)[-1] == 'narrow'
        else:
            assert lit._flat is None and lit._opt is not None
        steps = []
        for _ in range(3):
            lit.training_step(batch, 0)
            steps.append((lit.logged["loss"], lit.logged["reconstruction_loss"], lit.logged["hypersphere_loss"]))
        logged[fused] = np.array(steps)
    print(logged)
    assert np.isfinite(logged[None]).all()
    np.testing.assert_allclose(logged[None], logged[False], rtol=1e-3)


def test_vae_wrapper_takes_the_flat_step_at_a_window_length():
    from coskad_amd.lit import LitVAE
    from coskad_amd.trainer import STSAETrainStep
    args, cfg = _args("spherical_vae_seg8.yaml", 8)
    assert cfg["dataset_seg_len"] == 8 and cfg["latent_dim"] == 8 and cfg["dir_name"].endswith("_seg8")
    torch.manual_seed(0)
    lit = LitVAE(args).cuda()
    lit.setup("fit")
    assert type(lit._flat) is STSAETrainStep and 'wide' not in _kinds(lit._flat.enc) + _kinds(lit._flat.dec)
    loss = lit.training_step([R.synthetic_clips(64, 2, 8, 17, seed=5), None, None, None], 0)
    assert np.isfinite(float(loss)) and np.isfinite(lit.logged["kl_loss"])
    args, _ = _args("spherical_vae_seg8.yaml", 8, fused_window=False)
    lit = LitVAE(args).cuda()
    lit.setup("fit")
    assert lit._flat is None


# ---- 7. the command line -------------------------------------------------------------------------------------------------------------------

def test_window_autoencoder_train_eval_cli(tmp_path):
    """train_COSKAD.py then eval_COSKAD.py on config/synthetic/euclidean_autoencoder_seg16.yaml, each a fresh child process"""
    name = "euclidean_autoencoder_seg16.yaml"
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", name)), Loader=yaml.FullLoader)
    assert cfg["dataset_seg_len"] == 16
    cfg.update(exp_dir=str(tmp_path / "ckpt"), ae_epochs=1)
    path = str(tmp_path / name)
    yaml.safe_dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(cmd):
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
        return r.stdout

    out = run([sys.executable, "train_COSKAD.py", "--config", path])
    hist = [ast.literal_eval(l) for l in out.splitlines() if l.startswith("{") and "epoch" in l]
    assert len(hist) == 1 and np.isfinite(hist[0]["validation_auc"]) and 0.0 <= hist[0]["validation_auc"] <= 1.0
    ckdir = os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"])
    ckpts = sorted(glob.glob(os.path.join(ckdir, "*.ckpt")))
    assert ckpts
    ck = torch.load(ckpts[-1], map_location="cpu", weights_only=False)
    assert tuple(ck["state_dict"]["model.decoder.model.3.gcn.A"].shape) == (16, 17, 17)
    p2 = str(tmp_path / "eval.yaml")
    yaml.safe_dump(dict(cfg, load_ckpt=os.path.basename(ckpts[-1])), open(p2, "w"))
    out = run([sys.executable, "eval_COSKAD.py", "--config", p2])
    m = re.search(r"final AUC score: ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    auc = float(m.group(1))
    assert np.isfinite(auc) and 0.0 <= auc <= 1.0
