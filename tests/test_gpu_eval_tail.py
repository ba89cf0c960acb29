"""GPU parity of the decoder-tail kernel (csrc/eval_tail_window.hip) against the fp64 formula on the CPU: every shape
through ops.layer_tail with guard bands around every destination and NaN around every operand, one-clip batches, the persistent
loop, the decoder models on the new route and without it, a fold that must not survive a training step, the fallbacks and the
Lightning-style wrappers."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from oracle import ref_scoring as RS
from test_gpu_eval_window import GUARD, NAN, ODD_GUARD, SENTINEL, _check, _guards_untouched, _inside, _layer_ref, _tables

pytestmark = pytest.mark.gpu

Co, CoP = 2, 16
SCORE_TOL = dict(rtol=2e-4, atol=1e-5)      # the score tolerance of test_gpu_end_to_end.py::test_decoder_wrappers_fit_and_score
SHAPES = [(T, V, Ci) for T in (8, 12, 16, 24) for V in (17, 25) for Ci in (16, 32)]


class _Tail:
    """one tail layer's operands on the device: `in` and `x` 16-byte aligned views between NaN guards, tables / weights / bias at odd
    4-byte offsets between NaN guards; wfold [2 Ci][16] and bias [16] as coskad_bn_fold_f32 lays them out for two output channels
    (the 14 dead columns hold NaN: the kernel must not read them into anything)"""

    def __init__(self, T, V, Ci, B, seed, slope_in, slope_out):
        g = torch.Generator().manual_seed(seed)
        self.T, self.V, self.Ci, self.B = T, V, Ci, B
        self.A, self.Tm = _tables(T, V, g)
        self.w = torch.randn(2 * Ci, Co, generator=g) / (2 * Ci) ** 0.5
        self.b = torch.randn(Co, generator=g) * 0.5
        self.slope_in = torch.full((1,), 0.25) if slope_in else None
        self.slope_out = torch.full((1,), 0.2) if slope_out else None
        self.inp = torch.randn(B, Ci, T, V, generator=g)
        self.ref = _layer_ref(self.inp, self.A, self.Tm, self.w, self.b, self.slope_in, self.slope_out)          # fp64
        # the target: the layer's own output + 0.5 randn, so that scores are O(0.25) and the absolute term carries nothing
        self.x = (self.ref + 0.5 * torch.randn(B, Co, T, V, generator=g).double()).float()
        self.score_ref = ((self.ref - self.x.double()) ** 2).reshape(B, -1).mean(-1)
        wfold = torch.full((2 * Ci, CoP), NAN)
        wfold[:, :Co] = self.w
        bias = torch.full((CoP,), NAN)
        bias[:Co] = self.b
        self.dev, self.parents = {}, {}
        for n, t, guard in (("A", self.A, ODD_GUARD), ("Tm", self.Tm, ODD_GUARD), ("wfold", wfold, ODD_GUARD), ("bias", bias, ODD_GUARD),
                            ("inp", self.inp, GUARD), ("x", self.x, GUARD)):
            self.dev[n], self.parents[n] = _inside(t, NAN, guard)
        assert self.dev["inp"].data_ptr() % 16 == 0 and self.dev["x"].data_ptr() % 16 == 0
        self.dev["slope_in"] = None if self.slope_in is None else self.slope_in.cuda()
        self.dev["slope_out"] = None if self.slope_out is None else self.slope_out.cuda()

    def run(self, want_out=True, want_score=True, clip=None):
        """-> (out on the CPU or None, score on the CPU or None): destinations between sentinels (`score` at an odd offset), checked"""
        from coskad_amd import ops
        d = self.dev
        inp, x = (d["inp"], d["x"]) if clip is None else (d["inp"][clip:clip + 1].clone(), d["x"][clip:clip + 1].clone())
        B = inp.shape[0]
        out = outp = score = scorep = None
        if want_out:
            out, outp = _inside(torch.full((B, Co, self.T, self.V), SENTINEL), SENTINEL)
            assert out.data_ptr() % 16 == 0
        if want_score:
            score, scorep = _inside(torch.full((B,), SENTINEL), SENTINEL, ODD_GUARD)
        o, s = ops.layer_tail(inp, d["A"], d["Tm"], d["wfold"], d["bias"], Co, in_slope=d["slope_in"], out_slope=d["slope_out"],
                              x=x if want_score else None, want_out=want_out, want_score=want_score, out=out, score=score)
        assert (o is out) and (s is score)
        if want_out:
            _guards_untouched(outp, SENTINEL, "out")
        if want_score:
            _guards_untouched(scorep, SENTINEL, "score")
        return (out.cpu() if want_out else None), (score.cpu() if want_score else None)

    def operands_untouched(self):
        for n, p in self.parents.items():
            _guards_untouched(p, NAN, n)

    def check(self, out, score):
        _check(out, self.ref)
        assert torch.isfinite(score).all()
        print("scores", score[:4].tolist(), "max rel err", float(((score.double() - self.score_ref) / self.score_ref).abs().max()))
        np.testing.assert_allclose(score.double().numpy(), self.score_ref.numpy(), **SCORE_TOL)


# ---- 1. every shape ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V,Ci", SHAPES)
def test_tail_matches_fp64(T, V, Ci):
    from coskad_amd import ops
    assert ops.layer_tail_ok(T, V, Ci, Co) or (T, V) in ops.LAYER_TAIL_OFF
    k = SHAPES.index((T, V, Ci))
    L = _Tail(T, V, Ci, 3, seed=T * 1000 + V * 10 + Ci, slope_in=k % 2 == 0, slope_out=(k // 2) % 2 == 0)
    assert 0.05 < float(L.score_ref.min()) and float(L.score_ref.max()) < 2.0
    out, score = L.run()
    L.operands_untouched()
    L.check(out, score)
    out2, score2 = L.run()
    assert torch.equal(out2, out) and torch.equal(score2, score), "two calls differ"
    none, score3 = L.run(want_out=False)
    assert none is None and torch.equal(score3, score), "a score-only call differs"
    out4, none = L.run(want_score=False)
    assert none is None and torch.equal(out4, out), "an out-only call differs"
    L.operands_untouched()


# ---- 2. one clip: the fewest (34 of 256 threads) and the most (150) vectors per clip -------------------------------------------------------

@pytest.mark.parametrize("T,V,Ci", [(8, 17, 16), (24, 25, 32)])
def test_one_clip(T, V, Ci):
    L = _Tail(T, V, Ci, 1, seed=T + V + Ci, slope_in=True, slope_out=True)
    out, score = L.run()
    L.operands_untouched()
    L.check(out, score)


# ---- 3. the persistent loop: B = 2 cap + 3 (cap = 1024: the largest input is 2051 x 77 KB = 158 MB) ----------------------------------------

@pytest.mark.parametrize("T,V,Ci", [(8, 17, 16), (24, 25, 32)])
def test_persistent_loop(T, V, Ci):
    from coskad_amd import _lib
    cap = _lib.lib().coskad_layer_tail_max_grid(T, V, Ci)
    assert 0 < cap <= 2048
    B = 2 * cap + 3
    L = _Tail(T, V, Ci, B, seed=T + V + Ci + 1, slope_in=True, slope_out=False)
    out, score = L.run()
    L.operands_untouched()
    L.check(out, score)
    for clip in (0, cap, B - 1):                            # a clip's results do not depend on the workgroup or round that forms them
        o1, s1 = L.run(clip=clip)
        assert torch.equal(o1[0], out[clip]) and torch.equal(s1[0], score[clip]), f"clip {clip} differs from a one-clip call"


# ---- 4. the models -----------------------------------------------------------------------------------------------------------------------

def _stsae(T, V, latent=8, seed=1, channels=(32, 16, 32), hid=64):
    from coskad_amd.models.sts.ae import STSAE
    st = R.init_stse_state(2, tuple(channels), hid, latent, T, V, seed=seed, decoder=True)
    st["c"] = torch.linspace(-0.2, 0.2, latent)
    g = torch.Generator().manual_seed(seed + 100)           # running statistics away from (0, 1), so that a wrong fold shows
    for k in st:
        if k.endswith("running_mean"):
            st[k] = 0.3 * torch.randn(st[k].shape, generator=g)
        elif k.endswith("running_var"):
            st[k] = 0.5 + 1.5 * torch.rand(st[k].shape, generator=g)
    m = STSAE(2, list(channels), hid, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    return m, st


def _oracle(x, st, hid, T, V):
    ste = {k: v.clone() for k, v in st.items()}
    with torch.no_grad():
        z = R.stse_encode(x, ste, training=False)
        xr = R.stsae_decode(z, ste, hid, T, V, training=False)
    return z, xr, ((xr.double() - x.double()) ** 2).reshape(x.shape[0], -1).mean(-1)


def _check_scores(got, ref, msg=""):
    print(msg, "scores", got[:3].tolist(), "ref", ref[:3].tolist())
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.numpy(), err_msg=msg, **SCORE_TOL)


@pytest.mark.parametrize("T,V,latent", [(8, 17, 8), (16, 25, 8), (24, 17, 8), (24, 25, 16)])
def test_model_on_both_routes(T, V, latent, monkeypatch):
    """(24, 25) with latent 16: `lowrank_fold_ok` is false there, the head of the decoder is rev_btlnk + run_stack"""
    from coskad_amd import engine, ops
    if latent == 16:
        assert not ops.lowrank_fold_ok(latent, T * V)
    x = R.synthetic_clips(5, T=T, V=V, seed=T + V)
    m, st = _stsae(T, V, latent)
    m.cuda().eval()
    z_ref, xr_ref, s_ref = _oracle(x, st, 64, T, V)
    calls = []
    real = ops.layer_tail
    monkeypatch.setattr(ops, "layer_tail", lambda *a, **k: (calls.append(k.get("want_score")), real(*a, **k))[1])
    with torch.no_grad():
        assert m._tail_layer(x.cuda()) is m.decoder.model[-1]
        z, s = m.reconstruction_scores(x.cuda())
        z2, xr = m(x.cuda())
        assert calls == [True, False]                       # the kernel served both
        np.testing.assert_allclose(z.cpu().numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)
        _check_scores(s, s_ref, "tail")
        assert torch.equal(z, z2)
        np.testing.assert_allclose(xr.cpu().numpy(), xr_ref.numpy(), rtol=1e-4, atol=1e-4)
        engine.EVAL_TAIL = False
        try:
            assert m._tail_layer(x.cuda()) is None
            z3, s3 = m.reconstruction_scores(x.cuda())
            _, xr3 = m(x.cuda())
        finally:
            engine.EVAL_TAIL = True
        assert calls == [True, False]
        _check_scores(s3, s_ref, "without the tail")
        np.testing.assert_allclose(xr3.cpu().numpy(), xr_ref.numpy(), rtol=1e-4, atol=1e-4)


def test_model_at_12_frames():
    """reconstruction_scores takes the kernel at 12 frames; forward keeps its tile-kernel chain, bit for bit, whatever the switch says"""
    from coskad_amd import engine
    T, V = 12, 17
    x = R.synthetic_clips(5, T=T, V=V, seed=9)
    m, st = _stsae(T, V)
    m.cuda().eval()
    _, _, s_ref = _oracle(x, st, 64, T, V)
    with torch.no_grad():
        assert m._tail_layer(x.cuda()) is not None
        _, s = m.reconstruction_scores(x.cuda())
        _check_scores(s, s_ref, "12 frames")
        _, xr_on = m(x.cuda())
        engine.EVAL_TAIL = False
        try:
            _, xr_off = m(x.cuda())
        finally:
            engine.EVAL_TAIL = True
    assert torch.equal(xr_on, xr_off)


# ---- 5. the fold ------------------------------------------------------------------------------------------------------------------------

def test_tail_fold_does_not_survive_a_training_step():
    from coskad_amd.trainer import STSAETrainStep
    T, V = 8, 17
    x = R.synthetic_clips(5, T=T, V=V, seed=3)
    m, st = _stsae(T, V)
    m.cuda().eval()
    with torch.no_grad():
        _, s_old = m.reconstruction_scores(x.cuda())        # folds and caches
    _check_scores(s_old, _oracle(x, st, 64, T, V)[2], "before the step")
    assert m.decoder.model[-1].__dict__["_fold_cache"]
    m.train()
    eng = STSAETrainStep(m, mode='ae', lr=1e-2, alpha=1e-6, lambda_=0.5, fused_window=True)
    eng.step(x.cuda())
    torch.cuda.synchronize()
    m.eval()
    with torch.no_grad():
        _, s_new = m.reconstruction_scores(x.cuda())
    st_new = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    s_ref = _oracle(x, st_new, 64, T, V)[2]
    assert float((s_ref - s_old.double().cpu()).abs().max()) > 1e-3, "the step changed nothing: the test shows nothing"
    _check_scores(s_new, s_ref, "after the step")


# ---- 6. fallbacks -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["narrow", "no_running_stats"])
def test_fallbacks(kind):
    import torch.nn as nn
    T, V = 8, 17
    x = R.synthetic_clips(4, T=T, V=V, seed=2).cuda()
    if kind == "narrow":
        m, _ = _stsae(T, V, channels=(8, 8, 16), hid=16)          # the decoder runs 16 -> 16 -> 8 -> 8 -> 2
        assert m.decoder.model[-1].in_channels == 8
    else:
        m, _ = _stsae(T, V)
        last = m.decoder.model[-1]
        last.tcn[1] = nn.BatchNorm2d(2, track_running_stats=False)
        last.residual[1] = nn.BatchNorm2d(2, track_running_stats=False)
    m.cuda().eval()
    with torch.no_grad():
        assert m._tail_layer(x) is None
        z, s = m.reconstruction_scores(x)
        z2, xr = m(x)
    assert torch.isfinite(s).all() and torch.equal(z, z2)
    assert torch.equal(s, ((xr - x) ** 2).reshape(4, -1).mean(-1))


# ---- 7. the wrappers --------------------------------------------------------------------------------------------------------------------

def _args(**kw):
    a = dict(num_coords=2, h_dim=64, latent_dim=8, dataset_seg_len=8, dropout=0, channels=[32, 16, 32], projector="linear",
             encoder_type="STS_GCN", hyperbolic=False, static_center=False, center_tolerance=1e-3, opt_lr=2e-3, alpha=1e-6,
             dataset_batch_size=256, dataset_num_transform=2, dataset_headless=False, dataset_kp18_format=False, smoothing=50,
             dataset_choice="UBnormal", validation=True, lambda_=0.01, phi=1.0, beta=1e-3, gamma=1e-2, distribution="ps", warmup_epochs=0)
    a.update(kw)
    return Namespace(**a)


def _raise(*a, **k):
    raise AssertionError("the decoder ran")


def test_autoencoder_wrapper_scores(monkeypatch):
    from coskad_amd.lit import LitAutoEncoder
    T, V = 8, 17
    torch.manual_seed(0)
    lit = LitAutoEncoder(_args()).cuda()
    lit.model.c.copy_(torch.linspace(-0.2, 0.2, 8))
    lit.model.eval()
    x = R.synthetic_clips(6, T=T, V=V, seed=4)
    st = {k: v.detach().cpu().clone() for k, v in lit.model.state_dict().items()}
    z, xr, _ = _oracle(x, st, 64, T, V)
    for kind in ('rec', 'rec+hyp', 'hyp'):
        lit.score_type = kind
        if kind == 'hyp':
            monkeypatch.setattr(lit.model, "decode", _raise)
        want = RS.rec_and_hy_window_scores(x.numpy(), xr.numpy(), z.numpy(), st["c"].numpy(), lit.rec_loss_weight, kind)
        with torch.no_grad():
            got = lit.window_scores_from_batch(x.cuda()).cpu()
        print(kind, got[:3].tolist(), want[:3].tolist())
        np.testing.assert_allclose(got.double().numpy(), want, err_msg=kind, **SCORE_TOL)


def test_vae_wrapper_scores_without_the_decoder(monkeypatch):
    import torch.nn.functional as F
    from coskad_amd.lit import LitVAE
    T, V = 8, 17
    torch.manual_seed(0)
    lit = LitVAE(_args()).cuda()
    lit.model.mean_vector.copy_(torch.linspace(-1.0, 1.0, 8).reshape(1, 8))
    lit.model.eval()
    x = R.synthetic_clips(6, T=T, V=V, seed=4).cuda()
    with torch.no_grad():
        torch.manual_seed(11)
        z = lit.model(x)[0]
        want = 1 - F.cosine_similarity(lit.model.mean_vector.expand_as(z), z)
        monkeypatch.setattr(lit.model, "decode", _raise)
        torch.manual_seed(11)
        got = lit.window_scores_from_batch(x)
    assert torch.equal(got, want)
