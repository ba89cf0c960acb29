"""Latents wider than 16 (16 < L <= 512) on the HIP path: the wide one-class heads (csrc/heads.hip, heads_wide.hip), the wide bottleneck
(csrc/btlnk_wide.hip), the flat train step, the Lightning-style wrappers, the CLI and two gloo ranks -- against the oracle
formulas (oracle/ref_cpu.py) with fp64 autograd for the gradients."""
import os
import socket
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64           # guard floats around every output buffer (out-of-bounds writes)
SENT = 12345.0


def _guarded(n, dev="cuda"):
    buf = torch.full((n + 2 * GUARD,), SENT, device=dev, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, name):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu()
    assert bool((g == SENT).all()), f"{name}: write outside the buffer"


def _call_head(kind, z, c, VI=None, acc=None, gram=None):
    """Raw C-ABI call with guarded outputs; -> dict of host tensors."""
    from coskad_amd import _lib, ops
    from coskad_amd._lib import call, i32, ptr
    import ctypes
    B, L = z.shape
    S = ops.head_slots(L)
    bufs = {k: _guarded(n) for k, n in (("dz", B * L), ("score", B), ("stats", S), ("zh", B * L))}
    ws = ops.head_ws(B, z.device, L)
    st = ops._stream()
    dz, score, stats, zh = (bufs[k][1] for k in ("dz", "score", "stats", "zh"))
    if kind == "mse":
        call("coskad_mse_head_f32", ptr(z), ptr(c), ptr(dz), ptr(score), ptr(stats), ptr(acc), ctypes.c_float(1.0), ptr(ws), i32(B), i32(L), st)
    elif kind == "maha":
        call("coskad_mahalanobis_head_f32", ptr(z), ptr(c), ptr(VI), ptr(dz), ptr(score), ptr(stats), ptr(acc), ptr(gram), i32(1),
             ctypes.c_float(1.0), ptr(ws), i32(B), i32(L), st)
    else:
        call("coskad_poincare_head_f32", ptr(z), ptr(c), ptr(dz), ptr(zh), ptr(score), ptr(stats), ptr(acc), ctypes.c_float(1.0),
             ptr(ws), i32(B), i32(L), st)
    torch.cuda.synchronize()
    for k, (b, _) in bufs.items():
        _guards_intact(b, f"{kind} {k}")
    return {k: bufs[k][1].cpu().clone() for k in bufs}


@pytest.mark.parametrize("L", [17, 32, 64, 100, 512])
@pytest.mark.parametrize("B", [1, 7, 1037, 4096])
def test_wide_heads_match_oracle(L, B):
    from coskad_amd import ops
    g = torch.Generator().manual_seed(L * 7 + B)
    z = (0.3 * torch.randn(B, L, generator=g)).float()
    c = (0.2 * torch.randn(L, generator=g)).float()
    zc, cc = z.cuda(), c.cuda()
    S = ops.head_slots(L)
    Lp = max(L, 16)
    zd = z.double().requires_grad_(True)
    # ---- Euclidean
    acc = torch.zeros(S, device="cuda")
    out = _call_head("mse", zc, cc, acc=acc)
    loss = R.mse_to_center(zd, c.double())
    (gz,) = torch.autograd.grad(loss, zd)
    np.testing.assert_allclose(float(out["stats"][0]), float(loss), rtol=2e-5)
    np.testing.assert_allclose(out["dz"].view(B, L).numpy(), gz.numpy(), rtol=2e-4, atol=1e-9)
    np.testing.assert_allclose(out["score"].numpy(), R.euclid_window_score(z.double(), c.double()).numpy(), rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(out["stats"][1:1 + L].numpy(), z.double().sum(0).numpy(), rtol=1e-4, atol=1e-4)
    assert float(out["stats"][Lp + 1]) == B
    np.testing.assert_allclose(float(out["stats"][Lp + 2]), float(z.double().norm(dim=1).sum()), rtol=1e-5)
    # acc accumulates across two calls; the centre follows from it
    _call_head("mse", zc, cc, acc=acc)
    np.testing.assert_allclose(acc[1:1 + L].cpu().numpy(), 2 * z.double().sum(0).numpy(), rtol=1e-4, atol=2e-4)
    assert float(acc[Lp + 1]) == 2 * B
    cen = ops.center_finalize(acc, 1e-3, L).cpu()
    np.testing.assert_allclose(cen.numpy(), R.clamp_center(z.double().mean(0), 1e-3).numpy(), rtol=1e-4, atol=2e-6)
    # a repeat call is bitwise equal
    again = _call_head("mse", zc, cc)
    for k in ("dz", "score"):
        assert torch.equal(again[k], out[k]), k
    assert torch.equal(again["stats"], out["stats"])
    # ---- Poincare (a centre inside the ball, |c| = 0.4: distances away from artanh's clamp)
    c = (0.4 * c / c.norm()).float()
    cc = c.cuda()
    acc = torch.zeros(S, device="cuda")
    out = _call_head("poincare", zc, cc, acc=acc)
    loss, zh = R.poincare_loss(zd, c.double())
    (gz,) = torch.autograd.grad(loss, zd)
    np.testing.assert_allclose(float(out["stats"][0]), float(loss), rtol=1e-4)
    np.testing.assert_allclose(out["dz"].view(B, L).numpy(), gz.numpy(), rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(out["zh"].view(B, L).numpy(), zh.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(out["score"].numpy(), R.dist(c.double()[None], zh.detach()).numpy(), rtol=1e-4, atol=1e-5)
    mid = ops.midpoint_finalize(acc, L).cpu()
    np.testing.assert_allclose(mid.numpy(), R.weighted_midpoint(zh.detach()).numpy(), rtol=1e-3, atol=1e-5)
    dist_only = ops.poincare_dist(out["zh"].view(B, L).cuda(), cc).cpu()
    np.testing.assert_allclose(dist_only.numpy(), out["score"].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ops.poincare_logmap0(out["zh"].view(B, L).cuda()).cpu().numpy(), R.logmap0(zh.detach()).numpy(),
                               rtol=1e-3, atol=1e-5)
    again = _call_head("poincare", zc, cc)
    assert torch.equal(again["dz"], out["dz"]) and torch.equal(again["stats"], out["stats"])
    # ---- Mahalanobis (a non-symmetric VI: the gradient is (VI + VI^T) d / (2 dist))
    A = torch.randn(L, L, generator=g) / L ** 0.5
    VI = (A @ A.T + 0.5 * torch.eye(L) + 0.01 * torch.randn(L, L, generator=g)).float()
    acc = torch.zeros(S, device="cuda")
    gram = torch.full((L, L), 0.5, device="cuda")
    out = _call_head("maha", zc, cc, VI=VI.cuda(), acc=acc, gram=gram)
    dist = R.mahalanobis(zd, c.double()[None], VI.double())
    loss = dist.mean()
    (gz,) = torch.autograd.grad(loss, zd)
    np.testing.assert_allclose(float(out["stats"][0]), float(loss), rtol=1e-4)
    np.testing.assert_allclose(out["score"].numpy(), dist.detach().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(out["dz"].view(B, L).numpy(), gz.numpy(), rtol=2e-3, atol=1e-7)
    np.testing.assert_allclose(gram.cpu().numpy(), 0.5 + (z.double().T @ z.double()).numpy(), rtol=1e-4, atol=2e-4)
    assert float(out["stats"][Lp + 1]) == B
    again = _call_head("maha", zc, cc, VI=VI.cuda())
    assert torch.equal(again["dz"], out["dz"]) and torch.equal(again["stats"], out["stats"])


@pytest.mark.parametrize("L", [17, 32, 64, 512])
@pytest.mark.parametrize("K", [13056, 19200, 1004])
def test_wide_bottleneck_matches_fp64_autograd(L, K):
    from coskad_amd import ops
    B = 1037 if L < 512 else 263
    g = torch.Generator().manual_seed(L + K)
    U = torch.randn(B, K, generator=g).float()
    W = (torch.randn(L, K, generator=g) / K ** 0.5).float()
    b = (0.1 * torch.randn(L, generator=g)).float()
    dz = torch.randn(B, L, generator=g).float()
    for with_slope in (False, True):
        slope = torch.tensor([0.25]) if with_slope else None
        Ud, Wd, bd = (t.double().requires_grad_(True) for t in (U, W, b))
        sd = slope.double().requires_grad_(True) if with_slope else None
        X = torch.nn.functional.prelu(Ud, sd) if with_slope else Ud
        zr = torch.nn.functional.linear(X, Wd, bd)
        grads = torch.autograd.grad(zr, [Ud, Wd, bd] + ([sd] if with_slope else []), dz.double())
        Uc, Wc, bc, sc = U.cuda(), W.cuda(), b.cuda(), (slope.cuda() if with_slope else None)
        z = ops.btlnk_fwd(Uc, Wc, bc, sc)
        np.testing.assert_allclose(z.cpu().numpy(), zr.detach().numpy(), rtol=1e-4, atol=2e-4)
        assert torch.equal(ops.btlnk_fwd(Uc, Wc, bc, sc), z)                    # bitwise-repeatable
        assert torch.equal(ops.btlnk_fwd(Uc[:7], Wc, bc, sc), z[:7])            # a clip's latent does not depend on its batch
        for accumulate in (False, True):
            dWb, dW = _guarded(L * K)
            dbb, db = _guarded(L)
            dsb, ds = _guarded(1)
            dUb, dU = _guarded(B * K)
            init = 0.5 if accumulate else 0.0
            for t in (dW, db, ds):
                t.fill_(init)
            ws = torch.empty(ops.btlnk_bwd_ws_bytes(B, K, L), dtype=torch.uint8, device="cuda")
            ops.btlnk_bwd(Uc, Wc, dz.cuda(), sc, dW.view(L, K), db, ds if with_slope else None, ws, dU=dU.view(B, K),
                          accumulate=accumulate)
            torch.cuda.synchronize()
            for buf, name in ((dWb, "dW"), (dbb, "db"), (dsb, "dslope"), (dUb, "dU")):
                _guards_intact(buf, name)
            np.testing.assert_allclose(dU.view(B, K).cpu().numpy(), grads[0].numpy(), rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(dW.view(L, K).cpu().numpy(), init + grads[1].numpy(), rtol=1e-4, atol=2e-4)
            np.testing.assert_allclose(db.cpu().numpy(), init + grads[2].numpy(), rtol=1e-4, atol=1e-4)
            if with_slope:
                np.testing.assert_allclose(float(ds[0]), init + float(grads[3]), rtol=1e-4, atol=1e-3)
            dU2 = torch.empty_like(Uc)
            dW2 = torch.full((L, K), init, device="cuda")
            ops.btlnk_bwd(Uc, Wc, dz.cuda(), sc, dW2, None, None, ws, dU=dU2, accumulate=accumulate)
            assert torch.equal(dU2, dU.view(B, K)) and torch.equal(dW2, dW.view(L, K))


def _stse(latent, projector="linear", hidden_layers=None, seed=1):
    from coskad_amd.models.sts.ae import STSE
    st = R.init_stse_state(2, (32, 16, 32), 64, latent, 12, 17, seed=seed)
    torch.manual_seed(seed)          # the mlp projector keeps its module initialisation: the same draws for every model built here
    m = STSE(2, [32, 16, 32], 64, latent, 12, 17, 'sts_gcn', projector, 'euclidean', 0.0,
             **({"projector_hidden_layers": hidden_layers} if hidden_layers else {}))
    if projector == "linear":
        st["c"] = torch.linspace(-0.2, 0.2, latent)
        m.load_state_dict(st, strict=True)
    return m


def test_wide_flat_step_matches_oracle_and_autograd_step():
    from coskad_amd.trainer import AutogradTrainStep, STSETrainStep, make_train_step
    L = 64
    x = R.synthetic_clips(96, seed=4)
    # first step vs the oracle
    m = _stse(L).cuda().train()
    eng = make_train_step(m, lr=1e-3, alpha=1e-4, head='euclidean')
    assert isinstance(eng, STSETrainStep)
    st = R.init_stse_state(2, (32, 16, 32), 64, L, 12, 17, seed=1)
    st["c"] = torch.linspace(-0.2, 0.2, L)
    params = {k: v.clone().requires_grad_(True) for k, v in st.items() if R.is_param_key(k) and v.is_floating_point()}
    sto = dict(st)
    sto.update(params)
    zr = R.stse_encode(x, sto, training=True)
    loss_h = R.mse_to_center(zr, st["c"])
    loss_h.backward()
    stats = eng.step(x.cuda())
    np.testing.assert_allclose(float(stats[0]), float(loss_h), rtol=1e-4)
    # the loss gradients of the step (the flat gradient buffer; the regulariser's term is folded into Adam) vs the oracle's autograd
    for k, p in params.items():
        if k.endswith(("tcn.0.bias", "residual.0.bias")) or k not in eng.fp.gviews:
            continue      # analytically zero gradient (bias in front of a train-mode BatchNorm)
        want = p.grad.numpy()
        np.testing.assert_allclose(eng.fp.gviews[k].cpu().numpy(), want, rtol=1e-3, atol=1e-4 * float(abs(want).max()) + 1e-9, err_msg=k)
    # three steps: flat step == autograd step on the same weights
    outs = []
    for cls in (STSETrainStep, AutogradTrainStep):
        m = _stse(L).cuda().train()
        e = cls(m, lr=1e-3, alpha=1e-4, head='euclidean')
        losses = [float(e.step(x.cuda())[0]) for _ in range(3)]
        outs.append((losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, float(e.reg_loss())))
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-5)
    np.testing.assert_allclose(outs[0][2], outs[1][2], rtol=1e-5)
    for k in outs[0][1]:
        if k.endswith(("tcn.0.bias", "residual.0.bias")):
            continue
        np.testing.assert_allclose(outs[0][1][k].float().numpy(), outs[1][1][k].float().numpy(), rtol=2e-3, atol=2e-5, err_msg=k)


def test_wide_flat_step_in_a_hip_graph_equals_the_eager_step():
    from coskad_amd.trainer import STSETrainStep
    x = R.synthetic_clips(64, seed=5).cuda()
    res = []
    for use_graph in (False, True):
        m = _stse(32).cuda().train()
        eng = STSETrainStep(m, lr=1e-3, alpha=1e-6, head='euclidean', use_graph=use_graph)
        # the captured step's first call also runs one eager warm-up step outside capture: 3 calls = 4 updates
        losses = [float(eng.step(x)[0]) for _ in range(3 if use_graph else 4)]
        res.append((losses, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    np.testing.assert_allclose(res[0][0][1:], res[1][0], rtol=1e-5)
    for k in res[0][1]:
        np.testing.assert_allclose(res[0][1][k].float().numpy(), res[1][1][k].float().numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_wide_mlp_projectors():
    from coskad_amd.trainer import AutogradTrainStep, STSETrainStep, make_train_step
    x = R.synthetic_clips(96, seed=6).cuda()
    # latent 32, mlp [32]: flat step (first Linear on the wide bottleneck, the block on mlp_head.hip) == autograd step
    outs = []
    for cls in (STSETrainStep, AutogradTrainStep):
        m = _stse(32, "mlp", seed=3).cuda().train()
        m.c.copy_(torch.linspace(-0.1, 0.1, 32))
        assert m.btlnk.hip_ok
        if cls is STSETrainStep:
            assert isinstance(make_train_step(m, lr=1e-3, alpha=1e-6, head='euclidean'), STSETrainStep)
        e = cls(m, lr=1e-3, alpha=1e-6, head='euclidean')
        outs.append(([float(e.step(x)[0]) for _ in range(3)], {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-4)
    for k in outs[0][1]:
        if k.endswith(("tcn.0.bias", "residual.0.bias", "btlnk.net.0.bias")) or "num_batches" in k:
            continue      # biases in front of a train-mode BatchNorm: zero gradient, torch Adam's noise moves them by +-lr
        np.testing.assert_allclose(outs[0][1][k].float().numpy(), outs[1][1][k].float().numpy(), rtol=5e-3, atol=5e-5, err_msg=k)
    # latent 128, mlp [128]: beyond mlp_head.hip -> AutogradTrainStep with the wide heads; the loss is finite and falls
    m = _stse(128, "mlp", seed=3).cuda().train()
    m.c.copy_(torch.full((128,), 0.05))
    assert not m.btlnk.hip_ok
    e = make_train_step(m, lr=1e-3, alpha=1e-6, head='euclidean')
    assert isinstance(e, AutogradTrainStep)
    losses = [float(e.step(x)[0]) for _ in range(6)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def _lit_args(**kw):
    a = dict(num_coords=2, h_dim=64, latent_dim=32, dataset_seg_len=12, dropout=0, channels=[32, 16, 32],
             projector="linear", encoder_type="STS_GCN", hyperbolic=False, static_center=False,
             center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6, dataset_batch_size=256, dataset_num_transform=2,
             dataset_headless=False, dataset_kp18_format=False, smoothing=50, dataset_choice="UBnormal", validation=True)
    a.update(kw)
    return Namespace(**a)


@pytest.mark.parametrize("mode", ["euclid_dynamic", "hyperbolic", "mahalanobis_static", "autoencoder"])
def test_wide_wrappers_fit_one_epoch(mode, tmp_path):
    from coskad_amd.lit import LitAutoEncoder, LitEncoder, Trainer
    from coskad_amd.utils.synthetic import batches, make_dataset
    torch.manual_seed(0)
    train, _ = make_dataset(n_scenes=2, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=False, seed=1)
    test, gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=80, num_transform=2, anomaly=True, seed=2)
    if mode == "autoencoder":
        args = _lit_args(lambda_=0.01, decoder_channels=[8, 8], use_decoder=True, use_vae=False, static_center=True)
        lit = LitAutoEncoder(args).cuda()
    else:
        args = _lit_args(hyperbolic=mode == "hyperbolic", static_center=mode == "mahalanobis_static",
                         distance="mahalanobis" if mode == "mahalanobis_static" else "euclidean")
        lit = LitEncoder(args).cuda()
    lit.gts = gts
    tr = Trainer(max_epochs=1, ckpt_dir=str(tmp_path))
    tr.fit(lit, lambda: batches(train, 256, shuffle=True, seed=0), lambda: batches(test, 512))
    assert len(tr.history) == 1 and 0.0 <= tr.history[-1]["validation_auc"] <= 1.0
    assert np.isfinite(tr.history[-1]["loss"])
    assert lit.model.latent_dim == 32 and torch.isfinite(lit.model.c).all()
    if mode == "mahalanobis_static":
        assert torch.isfinite(lit.model.inv_cov_matrix).all() and float(lit.model.inv_cov_matrix.abs().sum()) > 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(cmd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    return r.stdout


def test_train_eval_cli_latent_64(tmp_path):
    """train_COSKAD.py then eval_COSKAD.py at latent_dim 64; the printed AUC equals the in-process AUC of the checkpoint."""
    import ast
    import glob
    import re
    import yaml
    from coskad_amd.lit import LitEncoder, Trainer
    from coskad_amd.utils.argparser import init_sub_args
    from coskad_amd.utils.synthetic import batches, make_dataset
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), ae_epochs=2, latent_dim=64)
    path = str(tmp_path / "wide.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    out = _run([sys.executable, "train_COSKAD.py", "--config", path])
    hist = [ast.literal_eval(l) for l in out.splitlines() if l.startswith("{") and "epoch" in l]
    assert len(hist) == 2 and all("validation_auc" in h for h in hist), out[-2000:]
    ckdir = os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"])
    ckpt = sorted(glob.glob(os.path.join(ckdir, "epoch=*-validation_auc=*.ckpt")))[-1]
    cfg2 = dict(cfg, load_ckpt=os.path.basename(ckpt))
    p2 = str(tmp_path / "eval.yaml")
    yaml.safe_dump(cfg2, open(p2, "w"))
    out2 = _run([sys.executable, "eval_COSKAD.py", "--config", p2])
    mm = re.search(r"final AUC score: ([0-9.eE+-]+)", out2)
    assert mm, out2[-2000:]
    auc_cli = float(mm.group(1))
    args, *_ = init_sub_args(Namespace(**dict(cfg, create_experiment_dir=False)))
    lit = LitEncoder(args).cuda()
    assert lit.model.latent_dim == 64
    test, gts = make_dataset(n_scenes=2, n_clips=3, n_persons=3, clip_len=200, num_transform=args.dataset_num_transform,
                             anomaly=True, seed=args.seed + 1)
    lit.gts = gts
    outs = Trainer().predict(lit, lambda: batches(test, args.dataset_batch_size), ckpt_path=ckpt)
    auc_here = float(lit.validation_epoch_end(outs))
    assert abs(auc_cli - auc_here) < 1e-6, (auc_cli, auc_here)
    assert 0.0 <= auc_cli <= 1.0


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from coskad_amd import parallel
    from coskad_amd.trainer import STSETrainStep
    x = R.synthetic_clips(48, seed=9)
    m = _stse(32).cuda().train()
    eng = STSETrainStep(m, lr=1e-3, alpha=0.0, head='euclidean')
    idx = parallel.shard_indices(48, rank, world)
    stats = eng.step(x[idx].cuda())
    c = eng.refresh_center(eps=1e-3).cpu()
    torch.cuda.synchronize()
    q.put((rank, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if v.is_floating_point()}, float(stats[0]), c.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_at_latent_32_agree():
    """Two ranks on one GPU (gloo): after a step and a centre refresh both hold the same parameters and the centre of the
    whole batch's latent sums (all-reduced wide accumulator)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, sd0, l0, c0), (_, sd1, l1, c1) = res
    assert np.isfinite([l0, l1]).all() and np.isfinite(c0).all() and c0.shape == (32,)
    np.testing.assert_array_equal(c0, c1)
    for k, v in sd0.items():
        if "running_var" in k or "running_mean" in k:
            continue      # per-rank BatchNorm statistics (the reference's DDP keeps them per rank)
        np.testing.assert_array_equal(v, sd1[k], err_msg=k)
