"""The decoder models (autoencoder, spherical VAE) at latents 17 .. 512 on the flat HIP step: the wide PowerSpherical head
(csrc/vae_head.hip, one wave per clip) against the float64 restatement, the three MFMA products of rev_btlnk (csrc/rev_btlnk_wide.hip) against
float64, the steps against the module surface, scoring, and the wrappers."""
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_refs import _GivenDirichlet, _ps_restatement_f64, _uniform_entropy_f64          # noqa: F401  (the PowerSpherical head in float64)

pytestmark = pytest.mark.gpu

SENT = -777.0


# ---- a. the PowerSpherical head ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [17, 65, 200, 512])
def test_wide_power_spherical_head_vs_float64(L):
    """B = 131 leaves the last block three clips; the concentration column sweeps the softplus and the identity region; rows 0 / 1 sit
    on the poles; inputs and outputs are column views of wider tensors (rows not 16-byte aligned), guard columns keep a sentinel; the
    float64 restatement on the same draws is the yardstick (the float32 one loses the KL to cancellation in lgamma at these widths)."""
    from coskad_amd import ops
    g = torch.Generator().manual_seed(5 + L)
    B = 131
    H2 = torch.randn(B, L + 1, generator=g)
    H2[:, L] = torch.linspace(-6, 25, B)
    H2[0, :L] = 0.0; H2[0, 0] = 3.0                       # mu = e1
    H2[1, :L] = 0.0; H2[1, 0] = -2.0                      # mu = -e1
    w = torch.randn(B, L, generator=g)
    w_kl, w_exp = 0.3 / B, 0.2 / B
    H2d, wd = H2.cuda(), w.cuda()
    torch.manual_seed(40 + L)
    z, kl, ik, saved = ops.ps_head_forward(H2d[:, :L], H2d[:, L:L + 1])
    out = torch.full((B, L + 3), SENT, device="cuda")      # guard columns 0 and L + 2 around the [B, L + 1] gradient
    ops.ps_head_backward(saved, wd, w_kl, w_exp, out[:, 1:L + 1], out[:, L + 1:L + 2])
    assert bool((out[:, 0] == SENT).all()) and bool((out[:, L + 2] == SENT).all())
    x, eps = saved[6], saved[7]
    assert eps.shape == (B, L - 1)
    z_ref, kl_ref, ik_ref, g_ref = _ps_restatement_f64(H2, x, eps, w, w_kl, w_exp)
    np.testing.assert_allclose(saved[2].cpu().numpy(), F.normalize(H2[:, :L].double(), dim=-1).numpy(), rtol=1e-5, atol=2e-7)
    np.testing.assert_allclose(z.cpu().numpy(), z_ref, rtol=1e-5, atol=2e-6)
    print("L", L, "max |kl - ref|", float(np.abs(kl.cpu().numpy() - kl_ref).max()), "kl range", float(kl_ref.min()), float(kl_ref.max()))
    np.testing.assert_allclose(kl.cpu().numpy(), kl_ref, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(ik.cpu().numpy(), ik_ref, rtol=1e-6)
    got = out[:, 1:L + 2].cpu().numpy()
    ok = np.isfinite(g_ref).all(axis=1)                    # (mu = e1 exactly: the restatement's own gradient is 0 / 0 there)
    assert ok.sum() >= B - 2
    print("L", L, "rows kept", int(ok.sum()), "max |grad - ref|", float(np.abs(got[ok] - g_ref[ok]).max()),
          "max |ref|", float(np.abs(g_ref[ok]).max()))
    np.testing.assert_allclose(got[ok], g_ref[ok], rtol=2e-3, atol=2e-6 + 2e-4 * np.abs(g_ref[ok]).max())
    # the same seed again: the same draws, and every output bit for bit
    torch.manual_seed(40 + L)
    z2, kl2, ik2, saved2 = ops.ps_head_forward(H2d[:, :L], H2d[:, L:L + 1])
    assert torch.equal(saved2[6], x) and torch.equal(saved2[7], eps)
    out2 = torch.full((B, L + 3), SENT, device="cuda")
    ops.ps_head_backward(saved2, wd, w_kl, w_exp, out2[:, 1:L + 1], out2[:, L + 1:L + 2])
    assert torch.equal(z2, z) and torch.equal(kl2, kl) and torch.equal(ik2, ik)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))     # (bit patterns: the pole row may hold a NaN)


# ---- b. rev_btlnk ------------------------------------------------------------------------------------------------------------------------
REV_SHAPES = [(37, 13056, 17), (5, 19200, 64), (130, 816, 200), (3, 13056, 512), (1030, 816, 33)]


def _no_fallback(monkeypatch):
    from coskad_amd import ops

    def refuse(*a, **k):
        raise AssertionError("the strided-GEMM fallback (cat / [N, L + 1] temporary / copies) ran at a wide latent")
    for name in ("gemm", "gemm_rows_outer"):
        monkeypatch.setattr(ops, name, refuse)


@pytest.mark.parametrize("route", ["wide", "fallback"])
@pytest.mark.parametrize("B,N,L", REV_SHAPES)
def test_wide_rev_btlnk_products_vs_float64(B, N, L, route, monkeypatch):
    """forward (with and without bias), dz (plain and added to a given one), dW / db (plain and accumulated) into views of a larger
    flat buffer with guard floats, against float64; ragged B, N, L; (1030, 816, 33) has more clips than a chunk.  `wide`: the MFMA
    kernels, which must not touch the GEMM fallback and repeat bit for bit; `fallback`: the branch ops.REV_WIDE_FALLBACK keeps."""
    from coskad_amd import ops
    assert ops.rev_btlnk_wide_ok(N, L) and not ops.rev_btlnk_ok(N, L)
    if route == "wide":
        _no_fallback(monkeypatch)
    else:
        monkeypatch.setattr(ops, "REV_WIDE_FALLBACK", {'fwd': frozenset({L}), 'bwd': frozenset({L})})
    g = torch.Generator().manual_seed(B + N + L)
    z = torch.randn(B, L, generator=g).cuda()
    W = (torch.randn(N, L, generator=g) / L ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    dH = torch.randn(B, N, generator=g).cuda()
    dz0 = torch.randn(B, L, generator=g).cuda()
    zd, Wd, dHd = z.double(), W.double(), dH.double()
    tol_f, tol_b = dict(rtol=1e-5, atol=1e-5), dict(rtol=2e-5, atol=2e-4)
    H = ops.rev_btlnk_fwd(z, W, b)
    np.testing.assert_allclose(H.cpu().numpy(), (zd @ Wd.t() + b.double()).float().cpu().numpy(), **tol_f)
    H0 = ops.rev_btlnk_fwd(z, W, None)
    np.testing.assert_allclose(H0.cpu().numpy(), (zd @ Wd.t()).float().cpu().numpy(), **tol_f)
    # the destinations: views into one flat buffer (as the step's gradient views), three guard floats around each
    G = 3
    flat = torch.full((G + N * L + G + N + G,), SENT, device="cuda")
    dW, db = flat[G:G + N * L].view(N, L), flat[2 * G + N * L:2 * G + N * L + N]
    dz = ops.rev_btlnk_bwd(dH, z, W, dW, db)
    ref_dz, ref_dW, ref_db = (dHd @ Wd).float().cpu().numpy(), (dHd.t() @ zd).float().cpu().numpy(), dHd.sum(0).float().cpu().numpy()
    np.testing.assert_allclose(dz.cpu().numpy(), ref_dz, **tol_b)
    np.testing.assert_allclose(dW.cpu().numpy(), ref_dW, **tol_b)
    np.testing.assert_allclose(db.cpu().numpy(), ref_db, **tol_b)
    guards = torch.cat([flat[:G], flat[G + N * L:2 * G + N * L], flat[-G:]])
    assert bool((guards == SENT).all())
    if route == "wide":                                     # fixed-order sums, no atomics: a second run gives the same bits
        keep = flat.clone()
        dz_again = ops.rev_btlnk_bwd(dH, z, W, dW, db)
        assert torch.equal(dz_again, dz) and torch.equal(flat, keep)
        assert torch.equal(ops.rev_btlnk_fwd(z, W, b), H)
        dW2 = torch.empty(N, L, device="cuda")
        ops.rev_btlnk_bwd(dH, z, W, dW2, None)              # no bias gradient asked for
        assert torch.equal(dW2, dW)
    dz1 = ops.rev_btlnk_bwd(dH, z, W, dW, db, dz=dz0.clone(), accumulate=True)
    np.testing.assert_allclose(dz1.cpu().numpy(), (dz0.double() + dHd @ Wd).float().cpu().numpy(), **tol_b)
    np.testing.assert_allclose(dW.cpu().numpy(), 2 * ref_dW, rtol=2e-5, atol=4e-4)
    np.testing.assert_allclose(db.cpu().numpy(), 2 * ref_db, rtol=2e-5, atol=4e-4)
    guards = torch.cat([flat[:G], flat[G + N * L:2 * G + N * L], flat[-G:]])
    assert bool((guards == SENT).all())


def test_wide_rev_btlnk_dz_does_not_depend_on_the_batch():
    """the N slices of the dz product depend on (N, L) only: a clip's dz is the same bits alone and inside a batch"""
    from coskad_amd import ops
    g = torch.Generator().manual_seed(3)
    B, N, L = 200, 816, 40
    z, W, dH = torch.randn(B, L, generator=g).cuda(), torch.randn(N, L, generator=g).cuda(), torch.randn(B, N, generator=g).cuda()
    dW = torch.empty(N, L, device="cuda")
    full = ops.rev_btlnk_bwd(dH, z, W, dW, None)
    part = ops.rev_btlnk_bwd(dH[130:137].contiguous(), z[130:137].contiguous(), W, dW, None)
    assert torch.equal(full[130:137], part)
    Hf, Hp = ops.rev_btlnk_fwd(z, W, None), ops.rev_btlnk_fwd(z[130:137].contiguous(), W, None)
    assert torch.equal(Hf[130:137], Hp)


# ---- c. the autoencoder step ------------------------------------------------------------------------------------------------------------
def _module_surface_ae(st, c, x, T, V, L, steps):
    from coskad_amd.models.sts.ae import STSAE
    m = STSAE(2, [32, 16, 32], 64, L, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st)
    m.c.copy_(c)
    m.cuda().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        z, xr = m(x)
        ps = [p for n, p in m.named_parameters() if 'bias' not in n]
        reg = 0.5 * sum((p ** 2).sum() for p in ps) / len(ps)
        (0.5 * ((xr - x) ** 2).mean() + ((z - m.c) ** 2).mean() + 1e-3 * reg).backward()
        opt.step()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("T,steps,fused", [(12, 2, False), (8, 1, True)])
def test_flat_autoencoder_step_latent_32_equals_torch_adam_on_the_module_surface(T, steps, fused):
    """latent 32: the flat step (wide bottleneck, MSE head, rev_btlnk on the MFMA kernels behind _PlainEntry, fused Adam) and the
    module-surface path (autograd + torch.optim.Adam) end with the same parameters; 12 frames two steps, 8 frames (`fused_window`) one."""
    from coskad_amd.models.sts.ae import STSAE
    from coskad_amd.trainer import STSAETrainStep, _PlainEntry
    from oracle import ref_cpu as R
    V, L, B = 17, 32, 24
    torch.manual_seed(13)
    proto = STSAE(2, [32, 16, 32], 64, L, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    st = {k: v.detach().clone() for k, v in proto.state_dict().items()}
    c = torch.linspace(-0.2, 0.2, L)
    x = R.synthetic_clips(B, 2, T, V, seed=14).cuda()
    m = STSAE(2, [32, 16, 32], 64, L, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st)
    m.c.copy_(c)
    m.cuda().train()
    eng = STSAETrainStep(m, mode='ae', lr=1e-3, alpha=1e-3, lambda_=0.5, fused_window=fused)
    assert type(eng.entry) is _PlainEntry and eng.lowrank is None
    if fused:
        assert 'window' in [s.kind for s in eng.enc.segs]
    for _ in range(steps):
        out = eng.step(x)
    torch.cuda.synchronize()
    assert out['z'].shape == (B, L)
    got = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref = _module_surface_ae(st, c, x, T, V, L, steps)
    for k in got:
        if k.endswith(("tcn.0.bias", "residual.0.bias")):
            continue        # analytically-zero gradients: autograd's rounding noise random-walks them under Adam
        np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), rtol=2e-3, atol=3e-4, err_msg=k)


# ---- d. the VAE step --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,projector,L,B", [(17, 'linear', 24, 24), (25, 'mlp', 24, 24), (17, 'linear', 511, 5)])
def test_flat_vae_step_wide_latent_matches_module_autograd(V, projector, L, B):
    """the flat step and the module-surface autograd path draw the same PowerSpherical sample under the same torch seed; losses and
    every gradient agree.  The KL is held to kl_ps_uniform in float64 on the module's (loc, scale): in float32 lgamma(alpha + beta)
    cancels at these widths."""
    from coskad_amd.models.sts.vae import PowerSpherical, STSVAE, kl_ps_uniform
    from coskad_amd.trainer import STSAETrainStep, _PlainEntry
    from oracle import ref_cpu as R
    torch.manual_seed(3)
    make = lambda: STSVAE(2, [32, 16, 32], 64, L, 12, V, 'sts_gcn', projector, 'euclidean', 0.0, distribution='ps')
    st = {k: v.detach().clone() for k, v in make().state_dict().items()}
    x = R.synthetic_clips(B, 2, 12, V, seed=4).cuda()
    phi, beta, gamma = 0.7, 0.3, 0.2
    m1 = make()
    m1.load_state_dict(st)
    m1.cuda().train()
    torch.manual_seed(11)
    z, xr, (q, p, kappa) = m1(x)
    l_rec, l_kl, l_exp = ((xr - x) ** 2).mean(), kl_ps_uniform(q, p).mean(), (1 / kappa).mean()
    (phi * l_rec + beta * l_kl + gamma * l_exp).backward()
    q64 = PowerSpherical(loc=q.loc.detach().double().cpu(), scale=q.scale.detach().double().cpu())
    l_kl64 = float((-q64.entropy() + _uniform_entropy_f64(L)).mean())      # kl_ps_uniform, all of it in float64
    m2 = make()
    m2.load_state_dict(st)
    m2.cuda().train()
    eng = STSAETrainStep(m2, mode='vae', lr=0.0, alpha=0.0, phi=phi, beta=beta, gamma=gamma)
    assert type(eng.entry) is _PlainEntry
    torch.manual_seed(11)
    out = eng.step(x)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out['z'].cpu().numpy(), z.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(out['rec']), float(l_rec), rtol=1e-4)
    print("KL: flat", float(out['head']), "float64", l_kl64, "module float32", float(l_kl))
    np.testing.assert_allclose(float(out['head']), l_kl64, rtol=1e-4)
    np.testing.assert_allclose(float(out['exp']), float(l_exp), rtol=1e-4)
    if projector == 'mlp':
        for (k1, b1), (k2, b2) in zip(m1.named_buffers(), m2.named_buffers()):
            if "btlnk" in k1:
                np.testing.assert_allclose(b2.cpu().numpy(), b1.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=k1)
    grads = {n: p.grad for n, p in m1.named_parameters()}
    gmax = max(float(v.abs().max()) for v in grads.values() if v is not None)
    for n, ref in grads.items():
        if ref is None:
            continue
        r = ref.cpu().numpy()
        d = eng.fp.gviews[n].cpu().numpy()
        print(n, "max|ref|", float(np.abs(r).max()), "max|diff|", float(np.abs(d - r).max()))
        np.testing.assert_allclose(d, r, rtol=2e-3, atol=2e-4 * np.abs(r).max() + 5e-5 * gmax, err_msg=n)


# ---- e. scoring --------------------------------------------------------------------------------------------------------------------------
def test_vae_eval_forward_head_on_hip_at_latent_32_equals_the_torch_head(monkeypatch):
    """STSVAE.forward in eval mode without autograd takes the head kernels at latent 32 too (csrc/vae_head.hip); with autograd
    enabled the same call runs the torch restatement: same seed -> same sample, reconstruction and concentration."""
    from coskad_amd import ops
    from coskad_amd.models.sts.vae import STSVAE
    from oracle import ref_cpu as R
    torch.manual_seed(7)
    m = STSVAE(2, [32, 16, 32], 64, 32, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0, distribution='ps').cuda().eval()
    x = R.synthetic_clips(40, 2, 12, 17, seed=9).cuda()
    calls = []
    real = ops.ps_head_forward
    monkeypatch.setattr(ops, "ps_head_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(21)
    with torch.no_grad():
        z1, r1, (q1, _, k1) = m(x)
    assert calls == [1]
    torch.manual_seed(21)
    z2, r2, (q2, _, k2) = m(x)
    assert calls == [1]
    np.testing.assert_allclose(k1.cpu().numpy(), k2.detach().cpu().numpy(), rtol=1e-4)
    np.testing.assert_allclose(q1.loc.cpu().numpy(), q2.loc.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(z1.cpu().numpy(), z2.detach().cpu().numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(r1.cpu().numpy(), r2.detach().cpu().numpy(), rtol=2e-4, atol=2e-5 * float(r2.abs().max()) + 1e-5)


def _lit_args(**kw):
    a = dict(num_coords=2, h_dim=64, latent_dim=32, dataset_seg_len=12, dropout=0, channels=[32, 16, 32],
             projector="linear", encoder_type="STS_GCN", hyperbolic=False, static_center=True,
             center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6, dataset_batch_size=256, dataset_num_transform=2,
             dataset_headless=False, dataset_kp18_format=False, smoothing=50, dataset_choice="UBnormal", validation=True,
             lambda_=0.01, phi=1.0, beta=1e-3, gamma=1e-2, distribution="ps", warmup_epochs=0, decoder_channels=[8, 8])
    a.update(kw)
    return Namespace(**a)


def test_autoencoder_window_scores_at_latent_32_equal_the_module_path(monkeypatch):
    """LitAutoEncoder.window_scores_from_batch at latent 32 (rev_btlnk's forward on the MFMA kernel through ops.rev_btlnk_fwd) against
    the CPU oracle's eval-mode encode / decode of the same weights"""
    from coskad_amd import ops
    from coskad_amd.lit import LitAutoEncoder
    from oracle import ref_cpu as R
    torch.manual_seed(0)
    lit = LitAutoEncoder(_lit_args(use_decoder=True, use_vae=False)).cuda()
    lit.model.c.copy_(torch.linspace(-0.2, 0.2, 32))
    lit.model.eval()
    x = R.synthetic_clips(9, 2, 12, 17, seed=4)
    seen = []
    real = ops.rev_btlnk_fwd
    monkeypatch.setattr(ops, "rev_btlnk_fwd", lambda z, W, b: (seen.append(tuple(z.shape)), real(z, W, b))[1])
    with torch.no_grad():
        got = lit.window_scores_from_batch(x.cuda()).cpu()
    assert seen == [(9, 32)]
    st = {k: v.detach().cpu().clone() for k, v in lit.model.state_dict().items()}
    with torch.no_grad():
        xr = R.stsae_decode(R.stse_encode(x, st, training=False), st, 64, 12, 17, training=False)
    want = ((xr - x) ** 2).reshape(x.shape[0], -1).mean(-1)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=1e-5)


# ---- f. the wrappers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["autoencoder", "spherical_vae"])
def test_wide_latent_wrappers_fit_on_the_flat_step(kind, tmp_path):
    from coskad_amd.lit import LitAutoEncoder, LitVAE, Trainer
    from coskad_amd.trainer import STSAETrainStep
    from coskad_amd.utils.synthetic import batches, make_dataset
    torch.manual_seed(0)
    train, _ = make_dataset(n_scenes=2, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=False, seed=1)
    test, gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=True, seed=2)
    cls = LitAutoEncoder if kind == "autoencoder" else LitVAE
    args = _lit_args(use_decoder=kind == "autoencoder", use_vae=kind == "spherical_vae")
    lit = cls(args).cuda()
    lit.gts = gts
    tr = Trainer(max_epochs=1, ckpt_dir=str(tmp_path))
    tr.fit(lit, lambda: batches(train, 256, shuffle=True, seed=0), lambda: batches(test, 512))
    assert type(lit._flat) is STSAETrainStep and lit._flat.steps > 0 and lit._opt is None
    assert len(tr.history) == 1 and 0.0 <= tr.history[-1]["validation_auc"] <= 1.0
    assert np.isfinite(tr.history[-1]["loss"]) and lit.model.latent_dim == 32
    # `flat_wide_latent: false` keeps the model on the autograd route
    off = cls(_lit_args(use_decoder=kind == "autoencoder", use_vae=kind == "spherical_vae", flat_wide_latent=False)).cuda()
    off.setup("fit", lambda: batches(train, 256, shuffle=False))
    assert off._flat is None and off._opt is not None
    # ... and changes nothing at a latent within 16
    narrow = cls(_lit_args(use_decoder=kind == "autoencoder", use_vae=kind == "spherical_vae", latent_dim=8, flat_wide_latent=False)).cuda()
    narrow.setup("fit", lambda: batches(train, 256, shuffle=False))
    assert type(narrow._flat) is STSAETrainStep
