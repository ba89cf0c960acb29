"""Gradient clipping, accumulation and optimiser state of the flat train steps (coskad_amd.trainer._FlatStep) against a yardstick
written out here: the module surface under autograd with loss = head + alpha * calc_reg_loss, torch.nn.utils.clip_grad_*, then
torch.optim.Adam.  Model and data of tests/test_gpu_modules.py::test_autograd_train_step_matches_fast_path_and_handles_mlp."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, ALPHA = 1e-3, 1e-4
ZERO_GRAD = ("tcn.0.bias", "residual.0.bias")      # conv biases in front of a train-mode BatchNorm: analytically zero gradient


def _stse():
    from coskad_amd.models.sts.ae import STSE
    from oracle import ref_cpu as R
    st = R.init_stse_state(2, (8, 4, 8), 8, 8, 12, 17, seed=1)
    st["c"] = torch.full((8,), 0.1)
    m = STSE(2, [8, 4, 8], 8, 8, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    return m.cuda().train()


_clips = {}


def clips(lo=0, hi=48):
    from oracle import ref_cpu as R
    if "x" not in _clips:
        _clips["x"] = R.synthetic_clips(48, seed=4).cuda()
    return _clips["x"][lo:hi].contiguous()


def flat(alpha=ALPHA, **kw):
    from coskad_amd.trainer import STSETrainStep
    m = _stse()
    return m, STSETrainStep(m, lr=LR, alpha=alpha, head='euclidean', **kw)


def reg_loss(m):
    ps = [p for n, p in m.named_parameters() if 'bias' not in n]
    return 0.5 * sum((p ** 2).sum() for p in ps) / len(ps)


class Yardstick:
    """autograd over the module surface, torch's clipping, torch's Adam"""

    def __init__(self, model=None, loss=None, alpha=ALPHA):
        self.alpha = alpha
        self.m = _stse() if model is None else model
        self.params = list(self.m.parameters())
        self.opt = torch.optim.Adam(self.params, lr=LR)
        self.loss = loss or (lambda m, x: torch.nn.functional.mse_loss(m(x), m.c.expand(x.shape[0], -1)))
        self.norm = None

    def backward(self, x, scale=1.0, reg_scale=None):
        """reg_scale: the regulariser's own weight where it is not the loss' (a deliberately wrong yardstick)"""
        reg_scale = scale if reg_scale is None else reg_scale
        (self.loss(self.m, x) * scale + self.alpha * reg_loss(self.m) * reg_scale).backward()

    def update(self, clip=0.0, mode='norm', frac=None):
        """frac: clip at that fraction of the total norm (mode 'norm') / at the median |g| (mode 'value') -> the clip value used"""
        self.norm = float(torch.nn.utils.clip_grad_norm_(self.params, 1e30))           # (a coefficient of 1: only the norm)
        if frac is not None:
            clip = frac * self.norm if mode == 'norm' else float(torch.cat([p.grad.reshape(-1) for p in self.params]).abs().median())
        if clip:
            (torch.nn.utils.clip_grad_norm_ if mode == 'norm' else torch.nn.utils.clip_grad_value_)(self.params, clip)
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return clip

    def moments(self, key):
        return {n: self.opt.state[p][key].detach().cpu().numpy() for n, p in self.m.named_parameters()}


def flat_moments(eng, buf):
    fp = eng.fp
    return {n: buf[fp.offsets[n]:fp.offsets[n] + fp.views[n].numel()].view(fp.views[n].shape).cpu().numpy() for n in fp.names}


def compared(names):
    return [n for n in names if not n.endswith(ZERO_GRAD)]


def check_params(m, ref_m, rtol=2e-3, atol=2e-5):
    ref = dict(ref_m.named_parameters())
    for n, p in m.named_parameters():
        if not n.endswith(ZERO_GRAD):
            np.testing.assert_allclose(p.detach().cpu().numpy(), ref[n].detach().cpu().numpy(), rtol=rtol, atol=atol, err_msg=n)


def grad_tol(ref, names, rtol):
    """the project's tolerance for gradient-like quantities (tests/test_gpu_modules.py:417) -> {name: (rtol, atol)}"""
    gmax = max(np.abs(ref[n]).max() for n in names)
    return {n: (rtol, 2e-4 * np.abs(ref[n]).max() + 5e-5 * gmax) for n in names}


def check_moments(eng, yard):
    for buf, key, rtol in ((eng.m, 'exp_avg', 2e-3), (eng.v, 'exp_avg_sq', 4e-3)):
        got, ref = flat_moments(eng, buf), yard.moments(key)
        names = compared(ref)
        for n, (rt, at) in grad_tol(ref, names, rtol).items():
            np.testing.assert_allclose(got[n], ref[n], rtol=rt, atol=at, err_msg=f"{key} {n}")


def bit_identical(a, b):
    (ma, ea), (mb, eb) = a, b
    assert torch.equal(ea.fp.flat, eb.fp.flat) and torch.equal(ea.m, eb.m) and torch.equal(ea.v, eb.v)
    sa, sb = ma.state_dict(), mb.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa if "running" not in k and "num_batches" not in k)


# ---- clipping --------------------------------------------------------------------------------------------------------------
def test_clipping_that_never_bites():
    """grad_clip_val = 1e30: parameters and moments bit-identical to a step built without clipping; last_grad_norm is the yardstick's
    total norm (so nothing stale and nothing that is no gradient sits in fp.grad)"""
    a, b = flat(), flat(grad_clip_val=1e30)
    a[1].step(clips()); b[1].step(clips())
    bit_identical(a, b)
    yard = Yardstick()
    yard.backward(clips())
    yard.update()
    got = float(b[1].last_grad_norm)
    print(f"grad norm: flat {got:.8g} yardstick {yard.norm:.8g}")
    np.testing.assert_allclose(got, yard.norm, rtol=2e-3)


@pytest.mark.parametrize("mode", ['norm', 'value'])
def test_clipping_that_bites(mode):
    """step 1 clipped (by norm: at 1 % of the yardstick's norm; by value: at its median |g|), set through set_gradient_clip; step 2
    with clipping off"""
    x = clips()
    yard, unclipped = Yardstick(), Yardstick()
    yard.backward(x); unclipped.backward(x)
    clip = yard.update(mode=mode, frac=0.01)
    unclipped.update()
    # the test discriminates only if the clip changes exp_avg by far more than the tolerance it is held at, in every compared tensor
    # (by value: in every tensor the clamp at least halves the largest element of -- a clamp at the median leaves a tensor whose
    # gradients all lie below it as it is, so "every tensor" cannot hold there: encoder.model.0.prelu.weight is such a one)
    ya, yb = yard.moments('exp_avg'), unclipped.moments('exp_avg')
    must = [n for n in compared(ya) if mode == 'norm' or np.abs(yb[n]).max() > 2 * 0.1 * clip]     # exp_avg = 0.1 g after step 1
    assert must
    for n, (rt, at) in grad_tol(ya, compared(ya), 2e-3).items():
        diff, tol = np.abs(ya[n] - yb[n]).max(), at + rt * np.abs(ya[n]).max()
        assert diff > 10 * tol or n not in must, f"{n}: clipped and unclipped yardsticks differ by {diff:.3g}, tolerance {tol:.3g}"
    m, eng = flat()
    eng.set_gradient_clip(clip, mode)
    eng.step(x)
    check_moments(eng, yard)
    eng.set_gradient_clip(0.0)
    eng.step(x)
    yard.backward(x)
    yard.update()
    check_moments(eng, yard)
    check_params(m, yard.m)


def test_clipping_under_use_graph_equals_eager_bit_for_bit():
    """three replayed steps == three eager steps with the same clip (the first graph-mode call takes the step twice on its input:
    an eager warm-up outside the capture, then the replay)"""
    xs = [clips(0, 32), clips(8, 40), clips(16, 48)]
    a, b = flat(grad_clip_val=1e-3), flat(grad_clip_val=1e-3, use_graph=True)
    for x in [xs[0]] + xs:
        a[1].step(x)
    for x in xs:
        b[1].step(x)
    torch.cuda.synchronize()
    assert float(a[1].last_grad_norm) > 1e-3                       # the clip bites
    print("max |dp| graph vs eager:", float((a[1].fp.flat - b[1].fp.flat).abs().max()))
    bit_identical(a, b)
    assert torch.equal(a[1].last_grad_norm, b[1].last_grad_norm)
    assert a[1].state_dict()['state'][0]['step'] == b[1].state_dict()['state'][0]['step'] == 4
    with pytest.raises(ValueError, match="captured"):
        b[1].set_gradient_clip(0.1)


# ---- accumulation ----------------------------------------------------------------------------------------------------------
def test_accumulate_two_halves_vs_yardstick():
    m, eng = flat(accumulate=2)
    yard = Yardstick()
    for lo in (0, 24):
        eng.step(clips(lo, lo + 24))
        yard.backward(clips(lo, lo + 24), 0.5)
    yard.update()
    assert eng.updates == 1 and eng._micro == 0
    check_params(m, yard.m)
    check_moments(eng, yard)
    ref = yard.m.state_dict()
    for k, v in m.state_dict().items():            # BatchNorm statistics stay per micro-batch
        if "running" in k or "num_batches" in k:
            np.testing.assert_allclose(v.cpu().numpy(), ref[k].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)


def test_accumulate_same_batch_twice_is_one_plain_step_bit_for_bit():
    """(g + g) * 0.5 is exact, and the plain step is the code as it was"""
    a, b = flat(), flat(accumulate=2)
    a[1].step(clips())
    b[1].step(clips()); b[1].step(clips())
    bit_identical(a, b)


def test_flush_applies_a_partial_group():
    """three micro-steps with accumulate = 2, then flush(): two updates, the second on the lone gradient scaled 1 / 2"""
    m, eng = flat(accumulate=2)
    yard = Yardstick()
    parts = [clips(0, 16), clips(16, 32), clips(32, 48)]
    for i, x in enumerate(parts):
        eng.step(x)
        yard.backward(x, 0.5)
        if i == 1:
            yard.update()
    assert eng.state_dict()['state'][0]['step'] == 1
    assert eng.flush() and not eng.flush()
    yard.update()
    sd = eng.state_dict()
    assert all(float(s['step']) == 2 for s in sd['state'].values()) and sd['coskad']['micro_step'] == 0
    check_params(m, yard.m)
    check_moments(eng, yard)


def test_flush_scales_the_regulariser_with_the_partial_group():
    """one micro-step of a group of two, then flush(): loss AND regulariser count 1 / 2, as on the autograd routes and under
    Lightning.  alpha = 100 makes the regulariser's gradient large enough for the project's tolerances to see its weight."""
    x = clips()
    yard, once = Yardstick(alpha=100.0), Yardstick(alpha=100.0)
    yard.backward(x, 0.5)
    once.backward(x, 0.5, reg_scale=1.0)          # what counting the regulariser once would give
    yard.update(); once.update()
    assert abs(once.norm - yard.norm) > 10 * 2e-3 * yard.norm, (once.norm, yard.norm)
    m, eng = flat(alpha=100.0, accumulate=2, grad_clip_val=1e30)
    eng.step(x)
    assert eng.flush()
    print(f"partial group: grad norm {float(eng.last_grad_norm):.8g}, yardstick {yard.norm:.8g}, regulariser once {once.norm:.8g}")
    np.testing.assert_allclose(float(eng.last_grad_norm), yard.norm, rtol=2e-3)
    check_moments(eng, yard)


def test_use_graph_with_accumulate_raises():
    with pytest.raises(ValueError, match="accumulate"):
        flat(accumulate=2, use_graph=True)
    for bad in (dict(grad_clip_val=-1.0), dict(grad_clip_val=float("nan")), dict(grad_clip_algorithm='l1'), dict(accumulate=0)):
        with pytest.raises(ValueError):
            flat(**bad)


# ---- the decoder step ------------------------------------------------------------------------------------------------------
def test_autoencoder_step_norm_clip_and_accumulate(golden):
    """STSAETrainStep on the smallest autoencoder of tests/test_gpu_ae_step.py: norm clip at 1 % of the yardstick's norm plus
    accumulate = 2, at that file's tolerances.  Two updates: after one update from zero moments the parameters move by lr * sign(g)
    whatever the clip coefficient and the 1 / k, so the first is held by the norm and the moments and only the second by the
    parameters."""
    from coskad_amd.models.sts.ae import STSAE
    from coskad_amd.trainer import STSAETrainStep
    from test_gpu_ae_step import _build
    g = golden("stsae_small.npz")
    x = torch.from_numpy(g["x"]).cuda()
    h = x.shape[0] // 2
    halves = [x[:h].contiguous(), x[h:].contiguous()]

    def model():
        m, st = _build(g, STSAE)
        m.load_state_dict(st, strict=True)
        m.c.copy_(torch.from_numpy(g["c"]))
        return m.cuda().train()

    def loss(m, xb):
        z, xr = m(xb)
        return 0.5 * ((xr - xb) ** 2).mean() + ((z - m.c) ** 2).mean()

    yard = Yardstick(model(), loss)
    for xb in halves:
        yard.backward(xb, 0.5)
    clip = yard.update(frac=0.01)
    m = model()
    eng = STSAETrainStep(m, mode='ae', lr=LR, alpha=ALPHA, lambda_=0.5, grad_clip_val=clip, accumulate=2)
    for xb in halves:
        eng.step(xb)
    assert eng.updates == 1
    np.testing.assert_allclose(float(eng.last_grad_norm), yard.norm, rtol=2e-3)
    check_moments(eng, yard)
    eng.set_gradient_clip(0.0)                     # second group unclipped: its gradient enters the moments at full size
    for xb in halves:
        eng.step(xb)
        yard.backward(xb, 0.5)
    yard.update()
    assert eng.updates == 2
    check_params(m, yard.m, rtol=2e-3, atol=3e-4)
    check_moments(eng, yard)


# ---- optimiser state -------------------------------------------------------------------------------------------------------
def test_checkpoint_interchange_with_torch_adam():
    """after two flat steps state_dict() loads into torch.optim.Adam(model.parameters()); one torch step from there equals one more
    flat step.  And back: torch's state after two yardstick steps loads into a flat step."""
    x = clips()
    m, eng = flat()
    eng.step(x); eng.step(x)
    sd = eng.state_dict()
    assert sorted(sd['state']) == list(range(len(eng.fp.names))) and sd['param_groups'][0]['params'] == sorted(sd['state'])
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'} and sd['param_groups'][0]['weight_decay'] == 0
    assert sd['param_groups'][0]['amsgrad'] is False and sd['param_groups'][0]['betas'] == (0.9, 0.999)
    for i, n in enumerate(eng.fp.names):
        assert sd['state'][i]['exp_avg'].shape == eng.fp.views[n].shape
    twin = _stse()
    twin.load_state_dict(m.state_dict(), strict=True)
    yard = Yardstick(twin)
    yard.opt.load_state_dict(sd)
    assert yard.opt.param_groups[0]['lr'] == LR
    yard.backward(x)
    yard.update()
    eng.step(x)
    check_params(m, yard.m)
    check_moments(eng, yard)
    # the reverse: a fresh flat step takes over from torch
    m2 = _stse()
    m2.load_state_dict(yard.m.state_dict(), strict=True)
    from coskad_amd.trainer import STSETrainStep
    eng2 = STSETrainStep(m2, lr=LR, alpha=ALPHA, head='euclidean')
    eng2.load_state_dict(yard.opt.state_dict())
    assert eng2.updates == 3
    np.testing.assert_allclose(float(eng2._bpow[0]), 0.9 ** 3, rtol=1e-6)
    eng2.step(x)
    yard.backward(x)
    yard.update()
    check_params(m2, yard.m)
    check_moments(eng2, yard)
    # own round trip: bit-exact continuation
    m3, eng3 = flat()
    m3.load_state_dict(m.state_dict(), strict=True)
    eng3.load_state_dict(eng.state_dict())
    eng.step(x); eng3.step(x)
    assert torch.equal(eng.fp.flat, eng3.fp.flat) and torch.equal(eng.m, eng3.m) and torch.equal(eng.v, eng3.v)
