"""GPU checks of the attribution axis: the folded layer's adjoint kernel (csrc/eval_layer_adj.hip) against float64
autograd of the oracle's eval-mode layer, its persistent loop and determinism, LitEncoder.window_attribution end to end against float64
autograd of the oracle's encoder and window scores for the three one-class heads, the frame-map kernel (csrc/attribution_frames.hip)
against its numpy yardstick, and eval_COSKAD.py --attribution-dir."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _check(got, ref, msg=""):
    """the project's tolerance (tests/test_gpu_eval_window.py): rtol 1e-4, atol 1e-4 of the reference's largest magnitude"""
    assert torch.isfinite(got).all(), msg + ": not every element was written"
    err = float((got.double() - ref).abs().max())
    print(f"{msg}: max |err| {err:.3e}, max |ref| {float(ref.abs().max()):.3e}")
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4 * float(ref.abs().max()), err_msg=msg)


# ---- 1. the kernel against fp64 autograd of the oracle's layer ----------------------------------------------------------------------

def _layer_state(T, V, Ci, Co, g):
    """one ST_GCNN layer in the oracle's state format (prefix `l`): random tables, convolutions, BatchNorm affine parameters AND
    running statistics; Ci == Co: identity residual (no residual keys)"""
    st = {"l.gcn.A": torch.randn(T, V, V, generator=g) * 0.3, "l.gcn.T": torch.randn(V, T, T, generator=g) * 0.3,
          "l.prelu.weight": torch.full((1,), 0.25)}
    for br, bn in (("tcn.0", "tcn.1"), ("residual.0", "residual.1")):
        if br.startswith("residual") and Ci == Co:
            continue
        st[f"l.{br}.weight"] = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
        st[f"l.{br}.bias"] = torch.randn(Co, generator=g) * 0.3
        st[f"l.{bn}.weight"] = 0.5 + torch.rand(Co, generator=g)
        st[f"l.{bn}.bias"] = torch.randn(Co, generator=g) * 0.3
        st[f"l.{bn}.running_mean"] = torch.randn(Co, generator=g) * 0.3
        st[f"l.{bn}.running_var"] = 0.5 + 1.5 * torch.rand(Co, generator=g)
        st[f"l.{bn}.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    return st


def _fold(st, dev="cuda"):
    """the layer's folded weights as layer_apply takes them: ops.bn_fold of the state"""
    from coskad_amd import ops

    def d(k):
        return st[k].to(dev).contiguous() if k in st else None

    def w2(k):
        return st[k].reshape(st[k].shape[0], -1).to(dev).contiguous() if k in st else None
    return ops.bn_fold(w2("l.tcn.0.weight"), d("l.tcn.0.bias"), d("l.tcn.1.weight"), d("l.tcn.1.bias"), d("l.tcn.1.running_mean"),
                       d("l.tcn.1.running_var"), w2("l.residual.0.weight"), d("l.residual.0.bias"), d("l.residual.1.weight"),
                       d("l.residual.1.bias"), d("l.residual.1.running_mean"), d("l.residual.1.running_var"))


def _ref_input_grad(st, x_in, dU, slope):
    """float64 autograd: d <U, dU> / d in, U = st_gcnn_layer(prelu(in)) before its own activation, eval mode"""
    st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in st.items()}
    x = x_in.double().requires_grad_(True)
    X = x if slope is None else R.prelu(x, slope.double())
    U = R.st_gcnn_layer(X, st64, "l", training=False, return_preact=True)
    (U * dU.double()).sum().backward()
    return x.grad


KERNEL_GEOMETRIES = [(8, 17), (12, 17), (16, 17), (12, 25), (24, 25)]
KERNEL_CHANNELS = [(2, 32), (32, 16), (16, 32), (32, 64), (16, 16), (32, 32)]     # (2, 32): the network input, no in_slope


def _kernel_case(T, V, Ci, Co, B=3):
    g = torch.Generator().manual_seed(T * 1000 + V * 10 + Ci + Co)
    st = _layer_state(T, V, Ci, Co, g)
    x_in = torch.randn(B, Ci, T, V, generator=g)
    x_in[torch.rand(B, Ci, T, V, generator=g) < 0.05] = 0.0         # exact zeros: PReLU' there is the slope
    assert (x_in == 0).any() and (x_in < 0).any() and (x_in > 0).any()
    dU = torch.randn(B, Co, T, V, generator=g)
    slope = None if Ci == 2 else torch.full((1,), 0.25)
    return st, x_in, dU, slope


@pytest.mark.parametrize("Ci,Co", KERNEL_CHANNELS)
@pytest.mark.parametrize("T,V", KERNEL_GEOMETRIES)
def test_kernel_matches_fp64_autograd(T, V, Ci, Co):
    from coskad_amd import ops
    assert ops.layer_input_grad_ok(T, V, Ci, Co)
    st, x_in, dU, slope = _kernel_case(T, V, Ci, Co)
    assert ("l.residual.0.weight" in st) == (Ci != Co)
    ref = _ref_input_grad(st, x_in, dU, slope)
    wfold, _ = _fold(st)
    out = torch.full((3, Ci, T, V), NAN, device="cuda")
    # (without a mask -- the network input -- x_in gives the shape and is not read: NaN there must not reach the result)
    xd = x_in.cuda() if slope is not None else torch.full_like(x_in, NAN).cuda()
    got = ops.layer_input_grad(dU.cuda(), xd, st["l.gcn.A"].cuda(), st["l.gcn.T"].cuda(), wfold, Co,
                               in_slope=None if slope is None else slope.cuda(), out=out)
    assert got is out
    _check(got.cpu(), ref, f"layer_input_grad {T}x{V} {Ci}->{Co}")


# ---- 2. the persistent loop -------------------------------------------------------------------------------------------------------

def test_persistent_loop_and_determinism():
    """B = the grid cap + 5: five workgroups go round twice.  The big batch repeats the three clips of the small one, so every clip's
    result -- whichever workgroup and round forms it -- must be the small run's, bit for bit."""
    from coskad_amd import ops
    T, V, Ci, Co = 8, 17, 16, 16
    cap = ops.layer_input_grad_max_grid(T, V, Ci, Co)
    assert cap in (256, 512)
    st, x_in, dU, slope = _kernel_case(T, V, Ci, Co)
    wfold, _ = _fold(st)
    A, Tm, sl = st["l.gcn.A"].cuda(), st["l.gcn.T"].cuda(), slope.cuda()
    small = ops.layer_input_grad(dU.cuda(), x_in.cuda(), A, Tm, wfold, Co, in_slope=sl)
    _check(small.cpu(), _ref_input_grad(st, x_in, dU, slope), "small batch")
    B = cap + 5
    idx = torch.arange(B) % 3
    big_dU, big_in = dU[idx].contiguous().cuda(), x_in[idx].contiguous().cuda()
    out = torch.full((B, Ci, T, V), NAN, device="cuda")
    big = ops.layer_input_grad(big_dU, big_in, A, Tm, wfold, Co, in_slope=sl, out=out)
    assert torch.equal(big[0], small[0])
    assert torch.equal(big, small[idx.cuda()]), "a clip's result depends on the workgroup or round that forms it"
    again = ops.layer_input_grad(big_dU, big_in, A, Tm, wfold, Co, in_slope=sl)
    assert torch.equal(again, big), "two runs differ"


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------

HEADS = ["euclidean", "poincare", "mahalanobis"]
E2E_GEOMETRIES = [(12, 17), (8, 17), (12, 25)]
LATENT = 16
_E2E_CACHE = {}


def _e2e_state(T, V, seed):
    st = R.init_stse_state(2, (32, 16, 32), 64, LATENT, T, V, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    for k in st:                                               # running statistics away from (0, 1), so that a wrong fold shows
        if k.endswith("running_mean"):
            st[k] = 0.3 * torch.randn(st[k].shape, generator=g)
        elif k.endswith("running_var"):
            st[k] = 0.5 + 1.5 * torch.rand(st[k].shape, generator=g)
    return st


def _masks(x, st, dtype):
    acts = []
    with torch.no_grad():
        R.stse_encode(x.to(dtype), {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}, training=False, collect=acts)
    return [a > 0 for a in acts]                               # PReLU keeps the sign: the mask of every hidden unit


def _e2e_inputs(T, V):
    """(state, x) of a geometry, with the precondition of the comparison CHECKED: the oracle's fp32 and fp64 PReLU masks agree at every
    hidden unit, so no element has to be left out (seeds are walked until one holds; the check runs on the CPU)"""
    if (T, V) not in _E2E_CACHE:
        for seed in range(1, 9):
            st, x = _e2e_state(T, V, seed), R.synthetic_clips(5, T=T, V=V, seed=seed + T + V)
            if all(torch.equal(a, b) for a, b in zip(_masks(x, st, torch.float32), _masks(x, st, torch.float64))):
                break
        else:
            raise AssertionError("no seed with equal fp32 / fp64 PReLU masks")
        _E2E_CACHE[(T, V)] = (st, x)
    return _E2E_CACHE[(T, V)]


def _head_tensors(head):
    g = torch.Generator().manual_seed(7)
    c = torch.linspace(-0.2, 0.2, LATENT)
    M = torch.randn(LATENT, LATENT, generator=g) * 0.2
    VI = M @ M.t() + 0.5 * torch.eye(LATENT)                   # symmetric positive definite
    return c, VI


def _oracle_scores(head, z, c, VI):
    if head == "euclidean":
        return R.euclid_window_score(z, c)
    if head == "poincare":
        return R.dist(c[None, :], R.project(R.expmap0(z)))
    return R.mahalanobis(z, c[None, :], VI)


def _lit(head, T, V, st, c, VI):
    from coskad_amd.lit import LitEncoder
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(dataset_seg_len=T, hyperbolic=head == "poincare", distance="mahalanobis" if head == "mahalanobis" else "euclidean")
    args, *_ = init_sub_args(Namespace(**cfg))
    lit = LitEncoder(args)
    # (the wrapper's joint count follows the dataset flags: 17; the 25-joint model is put in its place)
    lit.model = STSE(2, [32, 16, 32], 64, LATENT, T, V, 'sts_gcn', 'linear', lit.distance, 0.0)
    sd = dict(st)
    sd["c"] = c.clone()
    if head == "mahalanobis":
        sd["inv_cov_matrix"] = VI.clone()
    lit.model.load_state_dict(sd, strict=True)
    lit.cuda()
    lit.model.eval()
    return lit


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("T,V", E2E_GEOMETRIES)
def test_window_attribution_matches_fp64_autograd(T, V, head):
    st, x = _e2e_inputs(T, V)
    c, VI = _head_tensors(head)
    st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in st.items()}
    x64 = x.double().requires_grad_(True)
    s_ref = _oracle_scores(head, R.stse_encode(x64, st64, training=False), c.double(), VI.double())
    s_ref.sum().backward()                                     # eval mode: no batch coupling, so this is every window's own gradient
    g_ref = x64.grad
    lit = _lit(head, T, V, st, c, VI)
    score, grad, attr = lit.window_attribution(x.cuda())
    assert score.shape == (5,) and grad.shape == (5, 2, T, V) and attr.shape == (5, T, V)
    _check(score.cpu(), s_ref.detach(), f"score {head} {T}x{V}")
    _check(grad.cpu(), g_ref, f"grad {head} {T}x{V}")
    with torch.no_grad():
        ws = lit.window_scores(lit.model(x.cuda()))
    _check(score.cpu(), ws.cpu().double(), f"score vs window_scores {head} {T}x{V}")
    assert torch.equal(attr, (x.cuda() * grad).sum(1))
    missing = (x == 0).all(1)
    assert missing.any() and bool((attr.cpu()[missing] == 0).all()), "a missing joint (an exact 0 in x) must get 0"
    score2, grad2, _ = lit.window_attribution(x.cuda())
    assert torch.equal(score2, score) and torch.equal(grad2, grad)
    one = lit.window_attribution(x[2:3].cuda())
    assert torch.equal(one[1][0], grad[2]), "a window's gradient depends on the batch it arrives in"


def test_window_attribution_refuses_train_mode_on_the_device():
    st, x = _e2e_inputs(12, 17)
    lit = _lit("euclidean", 12, 17, st, *_head_tensors("euclidean"))
    lit.model.train()
    with pytest.raises(ValueError, match="train mode"):
        lit.window_attribution(x.cuda())


# ---- 4. the frame maps --------------------------------------------------------------------------------------------------------------

def test_frame_maps_equal_the_numpy_loop():
    from coskad_amd.utils import eval_utils
    from coskad_amd.utils.synthetic import make_dataset
    # (anomaly=False: the generator places a 30-frame anomaly in clips of more than 70 frames only)
    (x, trans, meta, frames), gts = make_dataset(n_scenes=1, n_clips=2, n_persons=2, clip_len=40, num_transform=2, anomaly=False)
    # person 1 of clip 2 enters late: its first frames are covered by no window -> NaN
    keep = ~((meta[:, 1] == 2) & (meta[:, 2] == 1) & (meta[:, 3] < 5))
    trans, meta, frames = trans[keep], meta[keep], frames[keep]
    N, T, V = frames.shape[0], frames.shape[1], 17
    attr = torch.randn(N, T, V, generator=torch.Generator().manual_seed(3))
    plan = eval_utils.ScorePlan(trans, meta, frames, gts, 2, device="cuda")
    want = eval_utils.attribution_frames(attr, frames, plan)
    got = eval_utils.attribution_frames_device(attr.cuda(), frames, plan)
    assert got.dtype == torch.float64 and tuple(got.shape) == (int(plan.row_ptr[-1]), V) == want.shape
    got = got.cpu().numpy()
    assert np.isnan(want).any() and not np.isnan(want).all()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got, want)                   # both sum in fp64 in the same order: exactly equal
    again = eval_utils.attribution_frames_device(attr.cuda(), frames.cuda(), plan).cpu().numpy()
    np.testing.assert_array_equal(again, got)


# ---- 5. the CLI -----------------------------------------------------------------------------------------------------------------------

def test_eval_cli_writes_the_maps(tmp_path):
    from coskad_amd.lit import LitEncoder, save_checkpoint
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), load_ckpt="init.ckpt", create_experiment_dir=False)
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(0)
    lit = LitEncoder(args).cuda()
    ckdir = os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"])
    os.makedirs(ckdir)
    save_checkpoint(lit, os.path.join(ckdir, "init.ckpt"))      # an untrained model: the test is about the files, not the score
    path = str(tmp_path / "eval.yaml")
    yaml.safe_dump(cfg, open(path, "w"))

    def run(*extra):
        r = subprocess.run([sys.executable, "eval_COSKAD.py", "--config", path, *extra], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return r.stdout
    plain, with_maps = run(), run("--attribution-dir", str(tmp_path / "maps"))
    final = re.findall(r"^final AUC score: \S+$", plain, flags=re.M)
    assert len(final) == 1 and re.findall(r"^final AUC score: \S+$", with_maps, flags=re.M) == final
    head = with_maps[:with_maps.index(final[0]) + len(final[0])]
    assert head == plain[:plain.index(final[0]) + len(final[0])]        # everything up to and including the AUC line is unchanged
    assert not os.path.exists(tmp_path / "maps" / "report.json")
    for sc in (1, 2):
        for cl in (1, 2, 3):
            a = np.load(tmp_path / "maps" / f"{sc}_{cl}_attribution.npy")
            p = np.load(tmp_path / "maps" / f"{sc}_{cl}_persons.npy")
            assert a.dtype == np.float32 and a.shape == (3, 200, 17) and p.tolist() == [0, 1, 2]
            assert np.isfinite(a).all() and np.abs(a).max() > 0           # every person is present in every frame of the synthetic clips
