"""GPU parity of the window lengths beside 12 (dataset_seg_len 8 / 16 / 24) against the CPU oracle: the mixing kernels of
csrc/gcn_window.hip through the C ABI, one composed layer, the encoder model and its flat train step, the decoder model through
its module surface, a Trainer run with scores and AUC, and the two command-line entry points."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import ref_cpu as R
from oracle import ref_scoring as RS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WINDOWS = [(T, V) for T in (8, 16, 24) for V in (14, 17, 18, 25)]
GUARD = 37            # floats on either side of a guarded tensor (odd: the views are 4-byte aligned, no more)
SENTINEL = -777.25


def _inside(t, fill):
    """a contiguous CUDA copy of t that is a view into the middle of a parent filled with `fill` -> (view, parent)"""
    parent = torch.full((t.numel() + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
    view = parent[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, parent


def _guards_untouched(parent, fill, name):
    g = torch.cat([parent[:GUARD], parent[-GUARD:]]).cpu()
    assert (torch.isnan(g).all() if fill != fill else (g == fill).all()), f"{name}: written outside the tensor"


def _tables(T, V, g):
    # 0.3 * randn: non-zero everywhere, so that a pad operand taken from a neighbour would show
    return torch.randn(T, V, V, generator=g) * 0.3, torch.randn(V, T, T, generator=g) * 0.3


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# rows = N * C.  (3, 2): 6 rows, less than one 16-row MFMA tile; (7, 9): 63 rows, the last tile is partial.  (8, 14) also on more
# than one round of the persistent grid: the mixing kernel takes 4 row tiles = 64 rows per workgroup pass there, on at most 512
# workgroups, so the (70, 256) = 17 920 rows of a first choice would be 280 passes, one round; (129, 256) = 33 024 rows are 516
# passes > 512, and the first four workgroups go round the grid-stride loop twice.
MIX_CASES = [(T, V, 3, 2) for T, V in WINDOWS] + [(8, 17, 7, 9), (24, 25, 7, 9), (16, 18, 7, 9), (8, 14, 129, 256)]


@pytest.mark.parametrize("T,V,N,C", MIX_CASES)
@pytest.mark.parametrize("adjoint", [False, True])
def test_window_gcn_matches_oracle(T, V, N, C, adjoint):
    from coskad_amd import _lib
    g = torch.Generator().manual_seed(T * 1000 + V * 10 + N)
    x = torch.randn(N, C, T, V, generator=g)
    A, Tm = _tables(T, V, g)
    if not adjoint:
        ref = R.gcn(x, A, Tm)
    else:
        xx = x.clone().requires_grad_(True)  # adjoint = vector-Jacobian product
        probe = torch.randn(N, C, T, V, generator=g)
        (R.gcn(xx, A, Tm) * probe).sum().backward()
        ref, x = xx.grad, probe
    nan = float("nan")
    (xd, xp), (Ad, Ap), (Td, Tp) = _inside(x, nan), _inside(A, nan), _inside(Tm, nan)
    out, outp = _inside(torch.full(x.shape, SENTINEL), SENTINEL)
    _lib.call("coskad_gcn_f32", _lib.ptr(xd), _lib.ptr(out), _lib.ptr(Ad), _lib.ptr(Td), _lib.i32(N * C), _lib.i32(T), _lib.i32(V),
              _lib.i32(1 if adjoint else 0), _stream())
    got = out.cpu()
    _guards_untouched(outp, SENTINEL, "out")
    for p, n in ((xp, "x"), (Ap, "A"), (Tp, "T")):
        _guards_untouched(p, nan, n)
    assert torch.isfinite(got).all()
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)


def _params_dx(x, dZ, A, Tm, dA, dT, dX, add, accumulate):
    from coskad_amd import _lib
    N, C, T, V = x.shape
    fn = _lib.lib().coskad_gcn_bwd_params_ws_bytes
    fn.restype = ctypes.c_size_t
    nbytes = fn(_lib.i32(T), _lib.i32(V))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.call("coskad_gcn_bwd_params_dx_f32", _lib.ptr(x), _lib.ptr(dZ), _lib.ptr(A), _lib.ptr(Tm), _lib.ptr(dA), _lib.ptr(dT),
              _lib.ptr(dX), _lib.ptr(add), _lib.ptr(ws), ctypes.c_size_t(nbytes), _lib.i32(1 if accumulate else 0), _lib.i32(N * C),
              _lib.i32(T), _lib.i32(V), _stream())


# the third row count is more than one round of the persistent grid.  (8, 17): two 16-row tiles per workgroup pass on 512 workgroups,
# 16 384 rows a round -> 129 * 128 = 16 512; (16, 17) (not asked for; the one geometry with two row tiles per pass in a 16-wave
# workgroup): 32 rows on 256 workgroups, 8 192 a round -> 65 * 128 = 8 320; the other three: 16 rows on 256 workgroups, 4 096 a
# round -> 65 * 64 = 4 160
PARAM_CASES = [(T, V, N, C) for T, V, big in ((8, 17, (129, 128)), (16, 25, (65, 64)), (24, 14, (65, 64)), (24, 25, (65, 64)),
                                             (16, 17, (65, 128)))
               for N, C in ((3, 2), (7, 9), big)]


@pytest.mark.parametrize("T,V,N,C", PARAM_CASES)
def test_window_gcn_bwd_params_dx(T, V, N, C):
    from coskad_amd import ops
    g = torch.Generator().manual_seed(T * 1000 + V * 10 + N)
    x = torch.randn(N, C, T, V, generator=g)
    dZ = torch.randn(N, C, T, V, generator=g)
    add = torch.randn(N, C, T, V, generator=g)
    A, Tm = _tables(T, V, g)
    dA0, dT0 = torch.randn(T, V, V, generator=g), torch.randn(V, T, T, generator=g)
    # fp64 autograd of the oracle's mixing, cast down
    x64, A64, T64 = (t.double().requires_grad_(True) for t in (x, A, Tm))
    (R.gcn(x64, A64, T64) * dZ.double()).sum().backward()
    want_A, want_T, want_X = A64.grad.float(), T64.grad.float(), x64.grad.float()
    nan = float("nan")
    (xd, xp), (zd, zp), (Ad, Ap), (Td, Tp), (addd, addp) = (_inside(t, nan) for t in (x, dZ, A, Tm, add))
    dx_two = ops.gcn(zd, Ad, Td, adjoint=True)           # the mixing kernel's adjoint: a second read of dZ

    def run(with_add, accumulate):
        # destinations: views of a larger buffer, as the flat gradient buffer hands them out
        (dA, dAp), (dT, dTp) = _inside(dA0, SENTINEL), _inside(dT0, SENTINEL)
        dX, dXp = _inside(torch.full(x.shape, SENTINEL), SENTINEL)
        _params_dx(xd, zd, Ad, Td, dA, dT, dX, addd if with_add else None, accumulate)
        for p, n in ((dAp, "dA"), (dTp, "dT"), (dXp, "dX")):
            _guards_untouched(p, SENTINEL, n)
        return dA.clone(), dT.clone(), dX.clone()

    for with_add, accumulate in ((False, False), (True, True), (True, False), (False, True)):
        dA, dT, dX = run(with_add, accumulate)
        dA2, dT2, dX2 = run(with_add, accumulate)
        assert torch.equal(dA, dA2) and torch.equal(dT, dT2) and torch.equal(dX, dX2), "two calls differ"
        for got, want, base, n in ((dA, want_A, dA0, "dA"), (dT, want_T, dT0, "dT")):
            w = (want + base) if accumulate else want
            assert torch.isfinite(got).all(), n
            np.testing.assert_allclose(got.cpu().numpy(), w.numpy(), rtol=1e-4, atol=1e-4 * float(want.abs().max()),
                                       err_msg=f"{n} add={with_add} accumulate={accumulate}")
        wx = dx_two + addd if with_add else dx_two
        np.testing.assert_allclose(dX.cpu().numpy(), wx.cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg="dX vs gcn(adjoint)")
        w64 = want_X + add if with_add else want_X
        np.testing.assert_allclose(dX.cpu().numpy(), w64.numpy(), rtol=1e-4, atol=1e-4 * float(w64.abs().max()), err_msg="dX")
    for p, n in ((xp, "x"), (zp, "dZ"), (Ap, "A"), (Tp, "T"), (addp, "add")):
        _guards_untouched(p, nan, n)
    # the parameter gradients alone (no dX)
    dA, dT = ops.gcn_bwd_params(xd, zd, Ad, Td)
    np.testing.assert_allclose(dA.cpu().numpy(), want_A.numpy(), rtol=1e-4, atol=1e-4 * float(want_A.abs().max()))
    np.testing.assert_allclose(dT.cpu().numpy(), want_T.numpy(), rtol=1e-4, atol=1e-4 * float(want_T.abs().max()))


# ---- one layer on the composed path ---------------------------------------------------------------------------------------------

def _layer_state(Ci, Co, T, V, seed, identity):
    g = torch.Generator().manual_seed(seed)
    st, p = {}, "L"
    st[p + ".gcn.A"] = (torch.rand(T, V, V, generator=g) * 2 - 1) / V ** 0.5
    st[p + ".gcn.T"] = (torch.rand(V, T, T, generator=g) * 2 - 1) / T ** 0.5
    for br, bn in (("tcn.0", "tcn.1"), ("residual.0", "residual.1")):
        if br.startswith("residual") and identity:
            continue
        st[f"{p}.{br}.weight"] = (torch.rand(Co, Ci, 1, 1, generator=g) * 2 - 1) / Ci ** 0.5
        st[f"{p}.{br}.bias"] = (torch.rand(Co, generator=g) * 2 - 1) / Ci ** 0.5
        st[f"{p}.{bn}.weight"] = 1 + 0.2 * torch.randn(Co, generator=g)
        st[f"{p}.{bn}.bias"] = 0.2 * torch.randn(Co, generator=g)
        st[f"{p}.{bn}.running_mean"] = torch.zeros(Co)
        st[f"{p}.{bn}.running_var"] = torch.ones(Co)
        st[f"{p}.{bn}.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    st[p + ".prelu.weight"] = torch.full((1,), 0.25)
    return st


ZERO_BIAS = ("tcn.0.bias", "residual.0.bias")     # conv biases in front of a train-mode BatchNorm: gradient exactly 0 here


def _check_grads(got: dict, want: dict):
    """test_layer_backward's tolerance: rtol 5e-4, atol 5e-5 max|want| + 2e-5 max over all gradients"""
    gmax = max(float(w.abs().max()) for k, w in want.items() if not k.endswith(ZERO_BIAS))
    checked = 0
    for k, w in want.items():
        a = got[k].detach().cpu().numpy()
        assert np.isfinite(a).all(), k
        if k.endswith(ZERO_BIAS):
            assert (a == 0).all(), k
            continue
        b = w.numpy().reshape(a.shape)
        np.testing.assert_allclose(a, b, rtol=5e-4, atol=5e-5 * max(float(np.abs(b).max()), 1e-9) + 2e-5 * gmax, err_msg=k)
        checked += 1
    return checked


def _check_running(got_state: dict, want_state: dict):
    n = 0
    for k, w in want_state.items():
        if k.endswith(("running_mean", "running_var")):
            np.testing.assert_allclose(got_state[k].cpu().numpy(), w.numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
            n += 1
        elif k.endswith("num_batches_tracked"):
            assert int(got_state[k]) == int(w), k
    return n


@pytest.mark.parametrize("T,V", [(8, 17), (24, 25)])
@pytest.mark.parametrize("Ci,Co,first", [(2, 32, True), (32, 16, False), (16, 16, False)])
def test_window_layer_forward_backward(T, V, Ci, Co, first):
    from coskad_amd.models.graph_layers.stsgcn import ST_GCNN_layer
    B, identity = 5, Ci == Co
    st = _layer_state(Ci, Co, T, V, seed=Ci * 100 + Co + T, identity=identity)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Ci, T, V, generator=g)
    probe = torch.randn(B, Co, T, V, generator=g)
    # oracle
    pk = [k for k in st if R.is_param_key(k) and st[k].is_floating_point()]
    stc = {k: v.clone() for k, v in st.items()}
    for k in pk:
        stc[k].requires_grad_(True)
    xo = x.clone().requires_grad_(not first)
    out_ref = R.st_gcnn_layer(xo, stc, "L", training=True)
    (out_ref * probe).sum().backward()
    # HIP: the module surface (forward_wide as one autograd node)
    layer = ST_GCNN_layer(Ci, Co, (1, 1), 1, T, V, 0.0)
    layer.load_state_dict({k[2:]: v for k, v in st.items()}, strict=True)
    layer.cuda().train()
    assert layer.is_wide
    xh = x.cuda().requires_grad_(not first)
    out = layer(xh)
    out.backward(probe.cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), out_ref.detach().numpy(), rtol=1e-4, atol=1e-4)
    got = {"L." + n: p.grad for n, p in layer.named_parameters()}
    assert _check_grads(got, {k: stc[k].grad for k in pk}) == len(pk) - (1 if identity else 2)
    assert _check_running({"L." + k: v for k, v in layer.state_dict().items()}, stc) == (2 if identity else 4)
    if not first:
        b = xo.grad.numpy()
        np.testing.assert_allclose(xh.grad.cpu().numpy(), b, rtol=5e-4, atol=5e-5 * float(np.abs(b).max()))


# ---- the encoder model and its flat train step ------------------------------------------------------------------------------------

def _stse(T, V=17, latent=16, seed=1):
    from coskad_amd.models.sts.ae import STSE
    st = R.init_stse_state(2, (32, 16, 32), 64, latent, T, V, seed=seed)
    st["c"] = torch.linspace(-0.2, 0.2, latent)
    m = STSE(2, [32, 16, 32], 64, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    return m, st


def _oracle_step(st, x, head):
    params = {k: v.clone().requires_grad_(True) for k, v in st.items() if R.is_param_key(k) and v.is_floating_point()}
    sto = {k: v.clone() for k, v in st.items()}
    sto.update(params)
    z = R.stse_encode(x, sto, training=True)
    loss = R.mse_to_center(z, st["c"]) if head == 'euclidean' else R.poincare_loss(z, st["c"])[0]
    loss.backward()
    return float(loss), {k: p.grad for k, p in params.items()}, sto


@pytest.mark.parametrize("T", [8, 16, 24])
def test_window_model_eval_and_train_step(T):
    from coskad_amd.trainer import STSETrainStep, make_train_step
    B = 5
    x = R.synthetic_clips(B, T=T, V=17, seed=T)
    m, st = _stse(T)
    m.cuda().eval()
    with torch.no_grad():
        z_eval = m(x.cuda()).cpu()
        z_ref = R.stse_encode(x, {k: v.clone() for k, v in st.items()}, training=False)
    np.testing.assert_allclose(z_eval.numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)
    loss_ref, grads_ref, sto = _oracle_step(st, x, 'euclidean')

    def one_step():
        m, _ = _stse(T)
        m.cuda().train()
        eng = make_train_step(m, lr=1e-3, alpha=1e-6, head='euclidean', use_graph=True)
        assert type(eng) is STSETrainStep and [s.kind for s in eng.stack.segs] == ['wide'] * 4
        stats = eng.step(x.cuda())
        torch.cuda.synchronize()
        return m, eng, stats

    m1, eng, stats = one_step()
    np.testing.assert_allclose(float(stats[0]), loss_ref, rtol=1e-4)
    assert set(grads_ref) == set(eng.fp.gviews)
    assert _check_grads(eng.fp.gviews, grads_ref) == len(grads_ref) - 8        # 4 tcn + 4 residual conv biases
    assert _check_running(m1.state_dict(), sto) == 16
    m2, eng2, stats2 = one_step()
    assert torch.equal(stats, stats2) and torch.equal(eng.fp.grad, eng2.fp.grad)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1), "two fresh steps from the same state differ"


def test_window_model_poincare_step():
    from coskad_amd.trainer import STSETrainStep, make_train_step
    T = 16
    x = R.synthetic_clips(5, T=T, V=17, seed=3)
    m, st = _stse(T)
    m.cuda().train()
    eng = make_train_step(m, lr=1e-3, alpha=1e-6, head='poincare')
    assert type(eng) is STSETrainStep
    stats = eng.step(x.cuda())
    loss_ref, _, _ = _oracle_step(st, x, 'poincare')
    np.testing.assert_allclose(float(stats[0]), loss_ref, rtol=1e-4)


# ---- decoder model: the module surface ----------------------------------------------------------------------------------------------

def test_window_autoencoder_modules():
    from argparse import Namespace
    from coskad_amd.lit import LitAutoEncoder
    from coskad_amd.models.sts.ae import STSAE
    T, V, B, hid, L = 8, 17, 4, 16, 8
    st = R.init_stse_state(2, (16, 8, 16), hid, L, T, V, seed=5, decoder=True)
    st["c"] = torch.linspace(-0.2, 0.2, L)
    x = R.synthetic_clips(B, T=T, V=V, seed=6)

    def model():
        m = STSAE(2, [16, 8, 16], hid, L, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
        m.load_state_dict(st, strict=True)
        return m.cuda()

    m = model().eval()
    with torch.no_grad():
        z, xr = m(x.cuda())
        ste = {k: v.clone() for k, v in st.items()}
        z_ref = R.stse_encode(x, ste, training=False)
        xr_ref = R.stsae_decode(z_ref, ste, hid, T, V, training=False)
    np.testing.assert_allclose(z.cpu().numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(xr.cpu().numpy(), xr_ref.numpy(), rtol=1e-4, atol=1e-4)
    # train mode: autograd through the module surface vs the oracle's
    params = {k: v.clone().requires_grad_(True) for k, v in st.items() if R.is_param_key(k) and v.is_floating_point()}
    sto = {k: v.clone() for k, v in st.items()}
    sto.update(params)
    zo = R.stse_encode(x, sto, training=True)
    xo = R.stsae_decode(zo, sto, hid, T, V, training=True)
    (((xo - x) ** 2).mean() + R.mse_to_center(zo, st["c"])).backward()
    m = model().train()
    xc = x.cuda()
    z, xr = m(xc)
    loss = ((xr - xc) ** 2).mean() + ((z - m.c[None]) ** 2).mean()
    loss.backward()
    got = {n: p.grad for n, p in m.named_parameters()}
    assert set(got) == set(params)
    assert _check_grads(got, {k: p.grad for k, p in params.items()}) == len(params) - 14
    assert _check_running(m.state_dict(), sto) == 28
    # the Lightning wrapper: a stack ending in a composed layer keeps the autograd optimiser
    args = Namespace(num_coords=2, h_dim=hid, latent_dim=L, dataset_seg_len=T, dropout=0, channels=[16, 8, 16], projector="linear",
                     encoder_type="STS_GCN", center_tolerance=1e-3, opt_lr=1e-3, alpha=1e-6, dataset_batch_size=64,
                     dataset_headless=False, dataset_kp18_format=False, dataset_choice="UBnormal", lambda_=0.01)
    lit = LitAutoEncoder(args).cuda()
    lit._make_optimiser('ae', lambda_=0.01)
    assert lit._flat is None and lit._opt is not None


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

def test_window_train_score_auc_parity(tmp_path):
    """tests/test_gpu_end_to_end.py::test_train_score_auc_parity in mode `euclid_dynamic` with 8-frame windows"""
    from argparse import Namespace
    from coskad_amd.lit import LitEncoder, Trainer
    from coskad_amd.utils.synthetic import batches, make_dataset
    torch.manual_seed(0)
    train, _ = make_dataset(n_scenes=2, n_clips=3, n_persons=2, clip_len=100, num_transform=2, anomaly=False, seed=1, T=8)
    test, gts = make_dataset(n_scenes=1, n_clips=3, n_persons=2, clip_len=100, num_transform=2, anomaly=True, seed=2, T=8)
    args = Namespace(num_coords=2, h_dim=16, latent_dim=8, dataset_seg_len=8, dropout=0, channels=[16, 8, 16],
                     projector="linear", encoder_type="STS_GCN", hyperbolic=False, static_center=False,
                     center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6, dataset_batch_size=256, dataset_num_transform=2,
                     dataset_headless=False, dataset_kp18_format=False, smoothing=50, dataset_choice="UBnormal", validation=True,
                     distance="euclidean")
    lit = LitEncoder(args).cuda()
    lit.gts = gts
    tr = Trainer(max_epochs=3, ckpt_dir=str(tmp_path))
    tr.fit(lit, lambda: batches(train, 256, shuffle=True, seed=0), lambda: batches(test, 512))
    auc = tr.history[-1]["validation_auc"]
    assert 0.0 <= auc <= 1.0 and len(tr.history) == 3
    st = {k: v.detach().cpu().clone() for k, v in lit.model.state_dict().items()}
    x, trans, meta, frames = test
    assert x.shape[2] == 8
    with torch.no_grad():
        z = R.stse_encode(x, st, training=False)
        s_ref = R.euclid_window_score(z, st["c"])
    auc_ref, per_t_ref, _ = RS.score_dataset(s_ref.double().numpy(), trans.numpy(), meta.numpy(), frames.numpy(), gts, 2)
    lit.model.eval()
    with torch.no_grad():
        z_hip = lit.model(x.cuda())
        s_hip = lit.window_scores(z_hip).cpu()
    np.testing.assert_allclose(z_hip.cpu().numpy(), z.numpy(), rtol=1e-4, atol=1e-4)           # latents: 1e-4
    tol = dict(rtol=2e-4, atol=1e-4)
    np.testing.assert_allclose(s_hip.numpy(), s_ref.numpy(), **tol)
    for t in per_t_ref:
        np.testing.assert_allclose(lit.last_scores[t], per_t_ref[t], **tol)                    # per-frame scores
    assert abs(auc - auc_ref) < 1e-2
    assert 1 <= len(glob.glob(str(tmp_path / "*.ckpt"))) <= 2


# ---- command line -------------------------------------------------------------------------------------------------------------------

def test_window_train_eval_cli(tmp_path):
    """train_COSKAD.py then eval_COSKAD.py on config/synthetic/euclidean_encoder_seg8.yaml, each a fresh child process"""
    import ast
    import re
    name = "euclidean_encoder_seg8.yaml"
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", name)), Loader=yaml.FullLoader)
    assert cfg["dataset_seg_len"] == 8
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
    assert tuple(ck["state_dict"]["model.encoder.model.0.gcn.A"].shape) == (8, 17, 17)
    p2 = str(tmp_path / "eval.yaml")
    yaml.safe_dump(dict(cfg, load_ckpt=os.path.basename(ckpts[-1])), open(p2, "w"))
    out = run([sys.executable, "eval_COSKAD.py", "--config", p2])
    m = re.search(r"final AUC score: ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    auc = float(m.group(1))
    assert np.isfinite(auc) and abs(auc - hist[0]["validation_auc"]) < 1e-6
