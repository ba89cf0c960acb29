"""GPU checks of the per-joint reconstruction-error maps: the map variant of the decoder-tail kernel
(csrc/eval_tail_window.hip through ops.layer_tail_map) against the fp64 formula with a derived per-element bound, its score against the
score-only launch bit for bit, the decomposition emap.sum() == score, one-clip batches, the persistent loop, the argument errors,
STSAE.reconstruction_map on both routes and on the fallbacks, the wrappers' window_error_map, LitAutoEncoder.window_latent_attribution
against float64 autograd of the oracle, the per-clip files against the numpy loop and eval_COSKAD.py --error-map-dir."""
import ast
import functools
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
from oracle import ref_scoring as RS
from test_gpu_eval_tail import SCORE_TOL, SHAPES, _Tail, _args, _oracle, _stsae
from test_gpu_eval_window import GUARD, ODD_GUARD, SENTINEL, _guards_untouched, _inside

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Co = 2


def _map_bound(xr_ref, x, rtol, atol):
    """The bound on |emap - ref| N (N = C T V) that follows from the tolerance delta_c = atol + rtol |x_rec_c| granted to the reconstruction
    itself: with d_c = x_rec_c - x_c in fp64 and the computed difference off by at most delta_c,
        |(d_c + e)^2 - d_c^2| <= delta_c (2 |d_c| + delta_c),   summed over the coordinates.
    -> (reference map [B, T, V] fp64, bound on the map [B, T, V] fp64)."""
    d = xr_ref.double() - x.double()
    delta = atol + rtol * xr_ref.double().abs()
    N = d.shape[1] * d.shape[2] * d.shape[3]
    return (d ** 2).sum(1) / N, (delta * (2 * d.abs() + delta)).sum(1) / N


def _check_map(emap, ref, bound, msg):
    emap = emap.detach().cpu()
    assert torch.isfinite(emap).all(), msg + ": not every element was written"
    assert bool((emap >= 0).all()), msg + ": a negative squared error"
    err = (emap.double() - ref).abs()
    print(f"{msg}: max |err| {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3e}, max ref {float(ref.max()):.3e}")
    assert bool((err <= bound).all()), msg


def _run_map(L, want_out=False, clip=None, guarded=True):
    """ops.layer_tail_map on the operands of a _Tail, destinations between sentinels (`emap` 16-byte aligned, `score` at an odd offset)
    -> (out or None, score, emap) on the CPU"""
    from coskad_amd import ops
    d = L.dev
    inp, x = (d["inp"], d["x"]) if clip is None else (d["inp"][clip:clip + 1].clone(), d["x"][clip:clip + 1].clone())
    B = inp.shape[0]
    out = outp = None
    if want_out:
        out, outp = _inside(torch.full((B, Co, L.T, L.V), SENTINEL), SENTINEL)
    score, scorep = _inside(torch.full((B,), SENTINEL), SENTINEL, ODD_GUARD)
    emap, emapp = _inside(torch.full((B, L.T, L.V), SENTINEL), SENTINEL)
    assert emap.data_ptr() % 16 == 0
    o, s, e = ops.layer_tail_map(inp, d["A"], d["Tm"], d["wfold"], d["bias"], Co, x, in_slope=d["slope_in"], out_slope=d["slope_out"],
                                 want_out=want_out, out=out, score=score, emap=emap)
    assert (o is out) and (s is score) and (e is emap)
    if want_out:
        _guards_untouched(outp, SENTINEL, "out")
    _guards_untouched(scorep, SENTINEL, "score")
    _guards_untouched(emapp, SENTINEL, "emap")
    return (out.cpu() if want_out else None), score.cpu(), emap.cpu()


@functools.lru_cache(maxsize=None)
def _case(T, V, Ci):
    """one tail layer per shape at B = 3 and its map launch with `out`: built once, shared by the tests below, left unchanged"""
    k = SHAPES.index((T, V, Ci))
    L = _Tail(T, V, Ci, 3, seed=T * 1000 + V * 10 + Ci, slope_in=k % 2 == 0, slope_out=(k // 2) % 2 == 0)
    return L, _run_map(L, want_out=True)


def _tail_bound(L):
    """delta: what test_gpu_eval_window._check grants `out` -- rtol 1e-4 and atol 1e-4 of the reference's largest magnitude"""
    return _map_bound(L.ref, L.x, 1e-4, 1e-4 * float(L.ref.abs().max()))


# ---- 1. the kernel against fp64 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V,Ci", SHAPES)
def test_map_matches_fp64(T, V, Ci):
    """|emap - ref| 2 T V <= sum_c delta_c (2 |d_c| + delta_c) per element, delta the tolerance of `out` (see _map_bound).  The operands
    sit between NaN guards and wfold / bias carry NaN in their 14 dead columns: a finite map has read none of them."""
    from coskad_amd import ops
    assert ops.layer_tail_ok(T, V, Ci, Co)
    L, (out, score, emap) = _case(T, V, Ci)
    L.operands_untouched()
    L.check(out, score)
    ref, bound = _tail_bound(L)
    assert tuple(emap.shape) == (3, T, V)
    _check_map(emap, ref, bound, f"emap {T}x{V} Ci={Ci}")


# ---- 2. the score is the existing score -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V,Ci", SHAPES)
def test_score_and_out_are_layer_tails(T, V, Ci):
    L, (out, score, emap) = _case(T, V, Ci)
    _, s_tail = L.run(want_out=False, want_score=True)
    assert torch.equal(score, s_tail), "the map launch's score differs from the score-only launch's"
    o_tail, _ = L.run(want_out=True, want_score=False)
    assert torch.equal(out, o_tail), "the map launch's reconstruction differs from layer_tail's"
    out2, score2, emap2 = _run_map(L, want_out=True)
    assert torch.equal(out2, out) and torch.equal(score2, score) and torch.equal(emap2, emap), "two calls differ"
    none, score3, emap3 = _run_map(L, want_out=False)
    assert none is None and torch.equal(score3, score) and torch.equal(emap3, emap), "a call without `out` differs"
    L.operands_untouched()


# ---- 3. the decomposition ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V,Ci", SHAPES)
def test_map_sums_to_the_score(T, V, Ci):
    """both are sums of the same 2 T V non-negative products in different orders plus one scaling each: rtol 4 T V 2^-24"""
    L, (_, score, emap) = _case(T, V, Ci)
    total = emap.double().sum((1, 2))
    print("sum", total.tolist(), "score", score.tolist())
    np.testing.assert_allclose(total.numpy(), score.double().numpy(), rtol=4 * T * V * 2.0 ** -24, atol=0)


# ---- 4. one clip: the fewest (34 of 256) and the most (150) storing threads -------------------------------------------------------------

@pytest.mark.parametrize("T,V,Ci", [(8, 17, 16), (24, 25, 32)])
def test_one_clip(T, V, Ci):
    L = _Tail(T, V, Ci, 1, seed=T + V + Ci, slope_in=True, slope_out=True)
    out, score, emap = _run_map(L, want_out=True)
    L.operands_untouched()
    L.check(out, score)
    _check_map(emap, *_tail_bound(L), f"one clip {T}x{V}")
    np.testing.assert_allclose(emap.double().sum((1, 2)).numpy(), score.double().numpy(), rtol=4 * T * V * 2.0 ** -24, atol=0)


# ---- 5. the persistent loop --------------------------------------------------------------------------------------------------------------

def test_persistent_loop():
    from coskad_amd import _lib
    T, V, Ci = 8, 17, 16
    cap = _lib.lib().coskad_layer_tail_max_grid(T, V, Ci)
    assert 0 < cap <= 2048
    B = 2 * cap + 3
    L = _Tail(T, V, Ci, B, seed=T + V + Ci + 1, slope_in=True, slope_out=False)
    _, score, emap = _run_map(L)
    L.operands_untouched()
    _check_map(emap, *_tail_bound(L), "persistent loop")
    assert torch.equal(score, L.run(want_out=False)[1])
    for clip in (0, cap, B - 1):                            # a clip's map does not depend on the workgroup or round that forms it
        _, s1, e1 = _run_map(L, clip=clip)
        assert torch.equal(s1[0], score[clip]) and torch.equal(e1[0], emap[clip]), f"clip {clip} differs from a one-clip call"


# ---- 6. argument errors -------------------------------------------------------------------------------------------------------------------

def test_argument_errors_name_the_operand_and_launch_nothing():
    from coskad_amd import _lib, ops
    T, V, Ci = 8, 17, 16
    L, _ = _case(T, V, Ci)
    d = L.dev
    score, scorep = _inside(torch.full((3,), SENTINEL), SENTINEL, ODD_GUARD)
    wide, widep = _inside(torch.full((3 * T * V + 4,), SENTINEL), SENTINEL)
    emap = wide[:3 * T * V].view(3, T, V)
    odd = wide[1:3 * T * V + 1].view(3, T, V)              # 4 bytes behind a 16-byte address
    assert emap.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 4

    def raw(x=d["x"], score=score, emap=emap, T=T, V=V, Ci=Ci):
        _lib.call("coskad_layer_tail_map_f32", d["inp"], x, None, score, emap, d["A"], d["Tm"], d["wfold"], d["bias"], None, None,
                  3, Ci, Co, T, V, ops._stream())

    for kw, name in ((dict(x=None), "`x`"), (dict(score=None), "`score`"), (dict(emap=None), "`emap`")):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*" + name + ".*NULL"):
            raw(**kw)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`emap`.*16-byte aligned"):
        raw(emap=odd)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`emap`.*16-byte aligned"):
        ops.layer_tail_map(d["inp"], d["A"], d["Tm"], d["wfold"], d["bias"], Co, d["x"], score=score, emap=odd)
    for kw in (dict(T=11), dict(V=14), dict(Ci=8)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\): unsupported layer_tail_map shape"):
            raw(**kw)
    narrow = torch.randn(3, 8, T, V, device="cuda")        # 8 input channels: outside layer_tail_ok
    with pytest.raises(_lib.CoskadHipError, match=r"layer_tail_map: unsupported shape .*C_in=8"):
        ops.layer_tail_map(narrow, d["A"], d["Tm"], torch.zeros(16, 16, device="cuda"), d["bias"], Co, d["x"], score=score, emap=emap)
    with pytest.raises(ValueError, match="x: tensor required"):
        ops.layer_tail_map(d["inp"], d["A"], d["Tm"], d["wfold"], d["bias"], Co, None)
    torch.cuda.synchronize()
    assert bool((score == SENTINEL).all()) and bool((wide == SENTINEL).all()), "a refused call wrote"
    _guards_untouched(scorep, SENTINEL, "score")
    _guards_untouched(widep, SENTINEL, "emap")


# ---- 7. the model ---------------------------------------------------------------------------------------------------------------------------

X_REC_TOL = dict(rtol=1e-4, atol=1e-4)      # test_gpu_eval_tail.py's tolerance of the models' x_rec: delta of the map bound here


def _check_scores(got, ref, msg):
    print(msg, "rec", got[:3].tolist(), "ref", ref[:3].tolist())
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.numpy(), err_msg=msg, **SCORE_TOL)


@pytest.mark.parametrize("T,V,latent", [(8, 17, 8), (16, 25, 8), (24, 25, 16), (12, 17, 8)])
def test_model_on_both_routes(T, V, latent, monkeypatch):
    """(24, 25) with latent 16: the head of the decoder is rev_btlnk + run_stack (no low-rank fold); 12 frames: forward keeps its
    tile-kernel chain, reconstruction_map takes the tail kernel"""
    from coskad_amd import engine, ops
    x = R.synthetic_clips(5, T=T, V=V, seed=T + V)
    m, st = _stsae(T, V, latent)
    m.cuda().eval()
    z_ref, xr_ref, s_ref = _oracle(x, st, 64, T, V)
    map_ref, bound = _map_bound(xr_ref, x, X_REC_TOL["rtol"], X_REC_TOL["atol"])
    xd = x.cuda()
    with torch.no_grad():
        assert m._tail_layer(xd) is m.decoder.model[-1]
        _, s_scores = m.reconstruction_scores(xd)
        calls = []
        real_map, real_tail = ops.layer_tail_map, ops.layer_tail
        monkeypatch.setattr(ops, "layer_tail_map", lambda *a, **k: (calls.append("map"), real_map(*a, **k))[1])
        monkeypatch.setattr(ops, "layer_tail", lambda *a, **k: (calls.append("tail"), real_tail(*a, **k))[1])
        z, rec, emap = m.reconstruction_map(xd)
        assert calls == ["map"], calls
        monkeypatch.undo()
        assert tuple(rec.shape) == (5,) and tuple(emap.shape) == (5, T, V)
        np.testing.assert_allclose(z.cpu().numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)
        assert torch.equal(rec, s_scores), "rec differs from reconstruction_scores' on the tail route"
        _check_scores(rec, s_ref, "tail")
        _check_map(emap, map_ref, bound, f"model {T}x{V} tail")
        engine.EVAL_TAIL = False
        try:
            assert m._tail_layer(xd) is None
            _, s_scores_off = m.reconstruction_scores(xd)
            _, rec_off, emap_off = m.reconstruction_map(xd)
        finally:
            engine.EVAL_TAIL = True
        assert torch.equal(rec_off, s_scores_off), "rec differs from reconstruction_scores' without the tail"
        _check_scores(rec_off, s_ref, "without the tail")
        _check_map(emap_off, map_ref, bound, f"model {T}x{V} without the tail")


@pytest.mark.parametrize("kind", ["narrow", "no_running_stats"])
def test_fallbacks_give_the_formula(kind):
    import torch.nn as nn
    T, V = 8, 17
    x = R.synthetic_clips(4, T=T, V=V, seed=2).cuda()
    if kind == "narrow":
        m, _ = _stsae(T, V, channels=(8, 8, 16), hid=16)          # the decoder's last layer has 8 input channels
        assert m.decoder.model[-1].in_channels == 8
    else:
        m, _ = _stsae(T, V)
        last = m.decoder.model[-1]
        last.tcn[1] = nn.BatchNorm2d(2, track_running_stats=False)
        last.residual[1] = nn.BatchNorm2d(2, track_running_stats=False)
    m.cuda().eval()
    with torch.no_grad():
        assert m._tail_layer(x) is None
        z, rec, emap = m.reconstruction_map(x)
        z2, xr = m(x)
        _, s = m.reconstruction_scores(x)
    assert torch.equal(z, z2) and torch.equal(rec, s)
    assert torch.equal(emap, ((xr - x) ** 2).sum(1) / (2 * T * V))


# ---- 8. the wrappers ------------------------------------------------------------------------------------------------------------------------

def test_autoencoder_wrapper():
    from coskad_amd.lit import LitAutoEncoder
    T, V = 8, 17
    torch.manual_seed(0)
    lit = LitAutoEncoder(_args()).cuda()
    lit.model.c.copy_(torch.linspace(-0.2, 0.2, 8))
    lit.model.eval()
    x = R.synthetic_clips(6, T=T, V=V, seed=4)
    st = {k: v.detach().cpu().clone() for k, v in lit.model.state_dict().items()}
    z, xr, _ = _oracle(x, st, 64, T, V)
    want = RS.rec_and_hy_window_scores(x.numpy(), xr.numpy(), z.numpy(), st["c"].numpy(), lit.rec_loss_weight, 'rec')
    map_ref, bound = _map_bound(xr, x, X_REC_TOL["rtol"], X_REC_TOL["atol"])
    lit.score_type = 'rec'
    with torch.no_grad():
        scores = lit.window_scores_from_batch(x.cuda())
    rec, emap = lit.window_error_map(x.cuda())
    assert tuple(rec.shape) == (6,) and tuple(emap.shape) == (6, T, V) and not emap.requires_grad
    assert torch.equal(rec, scores), "rec differs from window_scores_from_batch under 'rec'"
    np.testing.assert_allclose(rec.double().cpu().numpy(), want, **SCORE_TOL)
    _check_map(emap, map_ref, bound, "LitAutoEncoder rec")
    np.testing.assert_allclose(emap.double().sum((1, 2)).cpu().numpy(), rec.double().cpu().numpy(), rtol=4 * T * V * 2.0 ** -24, atol=0)
    lit.score_type = 'rec+hyp'                               # the map is of the reconstruction term, unscaled
    rec2, emap2 = lit.window_error_map(x.cuda())
    assert torch.equal(rec2, rec) and torch.equal(emap2, emap)
    lit.score_type = 'hyp'
    with pytest.raises(ValueError, match="'hyp'.*window_latent_attribution"):
        lit.window_error_map(x.cuda())
    lit.score_type = 'rec'
    lit.model.train()
    with pytest.raises(ValueError, match="train mode"):
        lit.window_error_map(x.cuda())


def test_vae_wrapper():
    from coskad_amd.lit import LitVAE
    T, V = 8, 17
    torch.manual_seed(0)
    lit = LitVAE(_args()).cuda()
    lit.model.mean_vector.copy_(torch.linspace(-1.0, 1.0, 8).reshape(1, 8))
    lit.model.eval()
    x = R.synthetic_clips(6, T=T, V=V, seed=4).cuda()
    with torch.no_grad():
        torch.manual_seed(11)
        xr = lit.model(x)[1]
    sq = (xr - x) ** 2
    torch.manual_seed(11)
    rec, emap = lit.window_error_map(x)
    # the same sampled latent, the same reconstruction: the kernel scales by the rounded 1 / (2 T V) where torch divides -- 3 roundings
    np.testing.assert_allclose(emap.cpu().numpy(), (sq.sum(1) / (2 * T * V)).cpu().numpy(), rtol=4 * 2.0 ** -24, atol=0)
    np.testing.assert_allclose(rec.double().cpu().numpy(), sq.reshape(6, -1).mean(-1).double().cpu().numpy(), **SCORE_TOL)
    lit.model.train()
    with pytest.raises(ValueError, match="train mode"):
        lit.window_error_map(x)


def test_encoder_wrapper_has_no_decoder():
    from coskad_amd.lit import LitEncoder
    lit = LitEncoder(_args()).cuda()
    lit.model.eval()
    with pytest.raises(ValueError, match="no decoder"):
        lit.window_error_map(torch.zeros(2, 2, 8, 17, device="cuda"))


# ---- 9. the latent term's input gradient ---------------------------------------------------------------------------------------------------------

LATENT = 16


def _masks(x, st, dtype):
    acts = []
    with torch.no_grad():
        R.stse_encode(x.to(dtype), {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}, training=False, collect=acts)
    return [a > 0 for a in acts]                               # PReLU keeps the sign: the mask of every hidden unit


def _ae_state(T, V):
    """(state, x) with the precondition of the comparison CHECKED: the oracle's fp32 and fp64 PReLU masks agree at every hidden unit of
    the encoder (seeds are walked until one holds; on the CPU)"""
    for seed in range(1, 9):
        st = R.init_stse_state(2, (32, 16, 32), 64, LATENT, T, V, seed=seed, decoder=True)
        g = torch.Generator().manual_seed(seed + 100)
        for k in st:                                           # running statistics away from (0, 1), so that a wrong fold shows
            if k.endswith("running_mean"):
                st[k] = 0.3 * torch.randn(st[k].shape, generator=g)
            elif k.endswith("running_var"):
                st[k] = 0.5 + 1.5 * torch.rand(st[k].shape, generator=g)
        st["c"] = torch.linspace(-0.2, 0.2, LATENT)
        x = R.synthetic_clips(5, T=T, V=V, seed=seed + T + V)
        if all(torch.equal(a, b) for a, b in zip(_masks(x, st, torch.float32), _masks(x, st, torch.float64))):
            return st, x
    raise AssertionError("no seed with equal fp32 / fp64 PReLU masks")


def _ae_lit(T, V, st=None, projector='linear'):
    from coskad_amd.lit import LitAutoEncoder
    from coskad_amd.models.sts.ae import STSAE
    lit = LitAutoEncoder(_args(dataset_seg_len=T, latent_dim=LATENT))
    # (the wrapper's joint count follows the dataset flags and it builds `linear` projectors: the model under test is put in its place)
    lit.model = STSAE(2, [32, 16, 32], 64, LATENT, T, V, 'sts_gcn', projector, 'euclidean', 0.0)
    if st is not None:
        lit.model.load_state_dict(st, strict=True)
    lit.cuda()
    lit.model.eval()
    return lit


def _check_grad(got, ref, msg):
    """tests/test_gpu_attribution.py::_check: rtol 1e-4, atol 1e-4 of the reference's largest magnitude"""
    assert torch.isfinite(got).all(), msg
    print(f"{msg}: max |err| {float((got.double() - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4 * float(ref.abs().max()), err_msg=msg)


@pytest.mark.parametrize("T,V", [(8, 17), (12, 25)])
def test_latent_attribution_matches_fp64_autograd(T, V):
    st, x = _ae_state(T, V)
    st64 = {k: (v.double() if v.is_floating_point() else v) for k, v in st.items()}
    x64 = x.double().requires_grad_(True)
    s_ref = R.euclid_window_score(R.stse_encode(x64, st64, training=False), st64["c"])
    s_ref.sum().backward()                                     # eval mode: no batch coupling, so this is every window's own gradient
    lit = _ae_lit(T, V, st)
    hyp, grad, attr = lit.window_latent_attribution(x.cuda())
    assert hyp.shape == (5,) and grad.shape == (5, 2, T, V) and attr.shape == (5, T, V)
    _check_grad(hyp.cpu(), s_ref.detach(), f"hyp {T}x{V}")
    _check_grad(grad.cpu(), x64.grad, f"grad {T}x{V}")
    assert torch.equal(attr, (x.cuda() * grad).sum(1))
    lit.score_type = 'hyp'
    with torch.no_grad():
        ws = lit.window_scores_from_batch(x.cuda())
    np.testing.assert_allclose(hyp.double().cpu().numpy(), ws.double().cpu().numpy(), **SCORE_TOL)
    one = lit.window_latent_attribution(x[2:3].cuda())
    assert torch.equal(one[1][0], grad[2]), "a window's gradient depends on the batch it arrives in"
    lit.model.train()
    with pytest.raises(ValueError, match="train mode"):
        lit.window_latent_attribution(x.cuda())


def test_latent_attribution_refusals():
    with pytest.raises(ValueError, match="projector 'mlp'"):
        _ae_lit(12, 17, projector='mlp').window_latent_attribution(torch.zeros(2, 2, 12, 17, device="cuda"))
    with pytest.raises(ValueError, match="V = 14"):
        _ae_lit(12, 14).window_latent_attribution(torch.zeros(2, 2, 12, 14, device="cuda"))


# ---- 10. the per-clip files --------------------------------------------------------------------------------------------------------------------

def test_files_equal_the_numpy_loop(tmp_path):
    from coskad_amd import attribution
    from coskad_amd.lit import LitAutoEncoder
    from coskad_amd.utils import eval_utils
    from coskad_amd.utils.synthetic import batches, make_dataset
    T, V = 8, 17
    (x, trans, meta, frames), gts = make_dataset(n_scenes=1, n_clips=2, n_persons=3, clip_len=30, num_transform=2, anomaly=False, T=T)
    # person 1 of clip 2 enters late: its first frames are covered by no window -> NaN
    keep = ~((meta[:, 1] == 2) & (meta[:, 2] == 1) & (meta[:, 3] < 5))
    data = (x[keep], trans[keep], meta[keep], frames[keep])
    torch.manual_seed(0)
    lit = LitAutoEncoder(_args()).cuda()
    lit.gts = gts
    lit.model.eval()
    loader = lambda: batches(data, 100)                      # several batches, the last one short
    outputs = [lit.predict_step(b, i) for i, b in enumerate(loader())]
    attribution.dataset_error_maps(lit, loader, outputs, str(tmp_path / "dev"))
    emap = torch.cat([lit.window_error_map(b[0])[1] for b in loader()], 0).cpu()
    plan = eval_utils.ScorePlan(data[1], data[2], data[3], gts, 2, device="cpu")
    eval_utils.save_attribution(str(tmp_path / "host"), eval_utils.attribution_frames(emap, data[3], plan), plan, suffix="error_map")
    names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / "dev" / "*")))
    assert names == ["1_1_error_map.npy", "1_1_persons.npy", "1_2_error_map.npy", "1_2_persons.npy"]
    seen_nan = False
    for n in names:
        a, b = np.load(tmp_path / "dev" / n), np.load(tmp_path / "host" / n)
        np.testing.assert_array_equal(a, b)                    # NaNs included
        if n.endswith("error_map.npy"):
            assert a.dtype == np.float32 and a.shape == (3, 30, V)
            seen_nan |= bool(np.isnan(a).any())
            assert (a[np.isfinite(a)] >= 0).all()
    assert seen_nan


# ---- 11. the command line --------------------------------------------------------------------------------------------------------------------------

def test_eval_cli_writes_the_error_maps(tmp_path):
    """train_COSKAD.py for one epoch on config/synthetic/euclidean_autoencoder.yaml, then eval_COSKAD.py --error-map-dir, each a fresh
    child process.  eval_COSKAD.py scores the autoencoder under 'hyp' unless the yaml's `eval_rec_loss_weight` says otherwise: the maps
    are asked for under 'rec+hyp'."""
    from coskad_amd.lit import LitEncoder, save_checkpoint
    from coskad_amd.utils.argparser import init_sub_args
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(*cmd, ok=True):
        r = subprocess.run([sys.executable, *cmd], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert (r.returncode == 0) == ok, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
        return r.stdout if ok else (r.stdout, r.stderr)

    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_autoencoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), ae_epochs=1)
    path = str(tmp_path / "train.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    out = run("train_COSKAD.py", "--config", path)
    assert len([ast.literal_eval(l) for l in out.splitlines() if l.startswith("{") and "epoch" in l]) == 1
    ckpts = sorted(glob.glob(os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"], "*.ckpt")))
    assert ckpts
    p2 = str(tmp_path / "eval.yaml")
    yaml.safe_dump(dict(cfg, load_ckpt=os.path.basename(ckpts[-1]), eval_rec_loss_weight=0.2), open(p2, "w"))
    plain = run("eval_COSKAD.py", "--config", p2)
    with_maps = run("eval_COSKAD.py", "--config", p2, "--error-map-dir", str(tmp_path / "maps"))
    final = re.findall(r"^final AUC score: \S+$", plain, flags=re.M)
    assert len(final) == 1 and re.findall(r"^final AUC score: \S+$", with_maps, flags=re.M) == final
    assert with_maps[:with_maps.index(final[0])] == plain[:plain.index(final[0])]      # everything up to the AUC line is unchanged
    for sc in (1, 2):
        for cl in (1, 2, 3):
            a = np.load(tmp_path / "maps" / f"{sc}_{cl}_error_map.npy")
            p = np.load(tmp_path / "maps" / f"{sc}_{cl}_persons.npy")
            assert a.dtype == np.float32 and a.shape == (3, 200, 17) and p.tolist() == [0, 1, 2]
            assert np.isfinite(a).all() and (a >= 0).all() and a.max() > 0     # every person is present in every frame of these clips
            assert not os.path.exists(tmp_path / "maps" / f"{sc}_{cl}_attribution.npy")
    # without the key the script scores under 'hyp', which has no reconstruction term: the wrapper's ValueError ends the run behind
    # the AUC line
    p_hyp = str(tmp_path / "eval_hyp.yaml")
    yaml.safe_dump(dict(cfg, load_ckpt=os.path.basename(ckpts[-1])), open(p_hyp, "w"))
    out, err = run("eval_COSKAD.py", "--config", p_hyp, "--error-map-dir", str(tmp_path / "hyp"), ok=False)
    assert len(re.findall(r"^final AUC score: \S+$", out, flags=re.M)) == 1
    assert "ValueError" in err and "'hyp'" in err and "window_latent_attribution" in err
    assert not glob.glob(str(tmp_path / "hyp" / "*"))
    # a one-class encoder has no decoder: likewise
    enc = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    enc.update(exp_dir=str(tmp_path / "enc"), load_ckpt="init.ckpt", create_experiment_dir=False)
    args, *_ = init_sub_args(Namespace(**enc))
    torch.manual_seed(0)
    ckdir = os.path.join(enc["exp_dir"], enc["dataset_choice"], enc["dir_name"])
    os.makedirs(ckdir)
    save_checkpoint(LitEncoder(args), os.path.join(ckdir, "init.ckpt"))
    p3 = str(tmp_path / "enc.yaml")
    yaml.safe_dump(enc, open(p3, "w"))
    out, err = run("eval_COSKAD.py", "--config", p3, "--error-map-dir", str(tmp_path / "none"), ok=False)
    assert len(re.findall(r"^final AUC score: \S+$", out, flags=re.M)) == 1
    assert "ValueError" in err and "no decoder" in err
    assert not glob.glob(str(tmp_path / "none" / "*"))
