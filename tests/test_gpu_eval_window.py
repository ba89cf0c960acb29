"""GPU parity of the folded one-clip layer kernel (csrc/eval_layer_clip.hip: 8 / 12 / 16 / 24 frames) against the fp64 formula on the
CPU: every layer shape through the C ABI, the persistent loop, the first pair; and at the window lengths 8 / 16 / 24 the encoder model
on the window route and on the composed one, a fold that must not survive a training step, and a decoder stack that mixes the routes."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

GEOMETRIES = [(T, V) for T in (8, 16, 24) for V in (17, 25)]
GUARD = 36            # floats on either side of a guarded tensor: a multiple of 4, so the views of `in` / `out` stay 16-byte aligned
ODD_GUARD = 37        # tables, weights, bias: 4-byte aligned views, no more
SENTINEL = -777.25
NAN = float("nan")


def _inside(t, fill, guard=GUARD):
    """a contiguous CUDA copy of t that is a view into the middle of a parent filled with `fill` -> (view, parent, guard)"""
    parent = torch.full((t.numel() + 2 * guard + 3,), fill, dtype=torch.float32, device="cuda")
    off = guard + (-(parent.data_ptr() // 4 + guard)) % 4 if guard % 4 == 0 else guard
    view = parent[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view, (parent, off, t.numel())


def _guards_untouched(pg, fill, name):
    parent, off, n = pg
    g = torch.cat([parent[:off], parent[off + n:]]).cpu()
    assert (torch.isnan(g).all() if fill != fill else (g == fill).all()), f"{name}: written outside the tensor"


def _tables(T, V, g):
    # 0.3 * randn: non-zero everywhere, so that a pad operand taken from a neighbour would show
    return torch.randn(T, V, V, generator=g) * 0.3, torch.randn(V, T, T, generator=g) * 0.3


def _prelu(x, a):
    return torch.where(x > 0, x, a * x)


def _layer_ref(x, A, Tm, wfold, bias, in_slope=None, out_slope=None):
    """fp64: U = Wz . gcn(X) + Wx . X + b, X = PReLU(x); wfold rows [0, Ci) act on gcn(X), rows [Ci, 2 Ci) on X"""
    X = x.double()
    if in_slope is not None:
        X = _prelu(X, float(in_slope))
    Ci = X.shape[1]
    Z = R.gcn(X, A.double(), Tm.double())
    W = wfold.double()
    U = torch.einsum("kc,bktv->bctv", W[:Ci], Z) + torch.einsum("kc,bktv->bctv", W[Ci:], X) + bias.double()[None, :, None, None]
    if out_slope is not None:
        U = _prelu(U, float(out_slope))
    return U


def _check(got, ref, msg=""):
    assert torch.isfinite(got).all(), msg
    np.testing.assert_allclose(got.double().numpy(), ref.numpy(), rtol=1e-4, atol=1e-4 * float(ref.abs().max()), err_msg=msg)


class _Layer:
    """one layer's operands on the device, every one a view between guards"""

    def __init__(self, T, V, Ci, Co, seed, slope_in, slope_out):
        g = torch.Generator().manual_seed(seed)
        self.A, self.Tm = _tables(T, V, g)
        self.wfold = torch.randn(2 * Ci, Co, generator=g) / (2 * Ci) ** 0.5
        self.bias = torch.randn(Co, generator=g) * 0.5
        self.slope_in = torch.full((1,), 0.25) if slope_in else None
        self.slope_out = torch.full((1,), 0.2) if slope_out else None
        self.g, self.Ci, self.Co, self.T, self.V = g, Ci, Co, T, V
        self.dev, self.parents = {}, {}
        for n in ("A", "Tm", "wfold", "bias"):
            self.dev[n], self.parents[n] = _inside(getattr(self, n), NAN, ODD_GUARD)
        self.dev["slope_in"] = None if self.slope_in is None else self.slope_in.cuda()
        self.dev["slope_out"] = None if self.slope_out is None else self.slope_out.cuda()

    def ref(self, x):
        return _layer_ref(x, self.A, self.Tm, self.wfold, self.bias, self.slope_in, self.slope_out)

    def run(self, xd):
        """-> (out view, its parent): through ops.layer_apply into a guarded destination"""
        from coskad_amd import ops
        B = xd.shape[0]
        out, outp = _inside(torch.full((B, self.Co, self.T, self.V), SENTINEL), SENTINEL)
        d = self.dev
        ops.layer_apply(xd, d["A"], d["Tm"], d["wfold"], d["bias"], self.Co, in_slope=d["slope_in"], out_slope=d["slope_out"], out=out)
        return out, outp

    def operands_untouched(self):
        for n, p in self.parents.items():
            _guards_untouched(p, NAN, n)


LAYER_CASES = [(T, V, Ci, Co) for T, V in GEOMETRIES + [(12, 17), (12, 25)] for Ci in (16, 32) for Co in (16, 32, 64)]


@pytest.mark.parametrize("T,V,Ci,Co", LAYER_CASES)
def test_layer_matches_fp64(T, V, Ci, Co):
    """(8, 17, *, 16): 9 position tiles, 3 per wave -- the fourth wave owns none"""
    from coskad_amd import ops
    assert ops.layer_apply_window_ok(T, V, Ci, Co) == (T != 12)
    first_half = LAYER_CASES.index((T, V, Ci, Co)) % 2 == 0
    L = _Layer(T, V, Ci, Co, seed=T * 1000 + V * 10 + Ci + Co, slope_in=first_half, slope_out=not first_half)
    x = torch.randn(3, Ci, T, V, generator=L.g)
    xd, xp = _inside(x, NAN)
    assert xd.data_ptr() % 16 == 0
    out, outp = L.run(xd)
    assert out.data_ptr() % 16 == 0
    got = out.cpu()
    _guards_untouched(outp, SENTINEL, "out")
    _guards_untouched(xp, NAN, "in")
    L.operands_untouched()
    _check(got, L.ref(x))
    out2, _ = L.run(xd)
    assert torch.equal(out2.cpu(), got), "two calls differ"


# the persistent grid: a workgroup takes clips blockIdx.x, blockIdx.x + grid, ..; grid = min(B, 256 CUs x workgroups per CU).
# (8, 17, 32 -> 32): 17.7 KB of image and 110 registers: 3 per CU, cap 768.  (24, 17, 32 -> 64): 52 KB of image (the 64 channels leave in
# two rounds through 32 rows) and 229 registers: 2 per CU, cap 512.  B = 2 cap + 3: three workgroups go round three times, the others
# twice, and the last round's prefetch finds no clip.  (12, 17, 32 -> 32) and (12, 25, 16 -> 32): the 12-frame choices are pinned
# where Geo<>'s rule would ask for 3 and for 2 per CU: 2 per CU, cap 512, and 3 per CU, cap 768.
LOOP_CASES = [(8, 17, 32, 32, 768), (24, 17, 32, 64, 512), (12, 17, 32, 32, 512), (12, 25, 16, 32, 768)]


@pytest.mark.parametrize("T,V,Ci,Co,cap", LOOP_CASES)
def test_persistent_loop(T, V, Ci, Co, cap):
    B = 2 * cap + 3
    L = _Layer(T, V, Ci, Co, seed=T + V + Ci + Co, slope_in=True, slope_out=False)
    x = torch.randn(B, Ci, T, V, generator=L.g)
    xd, xp = _inside(x, NAN)
    out, outp = L.run(xd)
    got = out.cpu()
    _guards_untouched(outp, SENTINEL, "out")
    _guards_untouched(xp, NAN, "in")
    _check(got, L.ref(x))
    for clip in (0, cap, B - 1):                            # a clip's output does not depend on the workgroup or round that forms it
        one, _ = L.run(xd[clip:clip + 1].clone())
        assert torch.equal(one.cpu()[0], got[clip]), f"clip {clip} differs from a one-clip call"


# first pair at (16, 25) -> 16: 38 rows = 61 KB of image: 2 per CU, cap 512; at (12, 25) -> 64: x, Y0, Z0 in rows 32..37 of the 64-row
# image: 2 per CU, cap 512
PAIR_CASES = ([(T, V, Co, 3) for T, V in GEOMETRIES + [(12, 17), (12, 25)] for Co in (16, 32, 64)]
              + [(16, 25, 16, 512 + 2), (12, 25, 64, 512 + 2)])


@pytest.mark.parametrize("T,V,Co,B", PAIR_CASES)
def test_first_pair_matches_fp64(T, V, Co, B):
    from coskad_amd import ops
    assert ops.layer_first_pair_ok(2, 32, Co, T, V)
    L1 = _Layer(T, V, 2, 32, seed=T * 100 + V + Co, slope_in=False, slope_out=False)
    L2 = _Layer(T, V, 32, Co, seed=T * 100 + V + Co + 1, slope_in=False, slope_out=False)
    mid = torch.full((1,), 0.25)
    has_out = Co != 32
    outs = torch.full((1,), 0.2) if has_out else None
    x = torch.randn(B, 2, T, V, generator=L1.g)
    h = _layer_ref(x, L1.A, L1.Tm, L1.wfold, L1.bias)
    ref = _layer_ref(h, L2.A, L2.Tm, L2.wfold, L2.bias, in_slope=mid, out_slope=outs)
    xd, xp = _inside(x, NAN)
    a, b = L1.dev, L2.dev

    def run():
        return ops.layer_first_pair_apply(xd, a["A"], a["Tm"], a["wfold"], a["bias"], b["A"], b["Tm"], b["wfold"], b["bias"], 32, Co,
                                          mid.cuda(), outs.cuda() if has_out else None)

    got = run().cpu()
    _guards_untouched(xp, NAN, "x")
    L1.operands_untouched()
    L2.operands_untouched()
    _check(got, ref)
    assert torch.equal(run().cpu(), got), "two calls differ"


# ---- the model ---------------------------------------------------------------------------------------------------------------------

def _stse(T, V, latent=16, seed=1, spread=True):
    from coskad_amd.models.sts.ae import STSE
    st = R.init_stse_state(2, (32, 16, 32), 64, latent, T, V, seed=seed)
    st["c"] = torch.linspace(-0.2, 0.2, latent)
    if spread:                                              # running statistics away from (0, 1), so that a wrong fold shows
        g = torch.Generator().manual_seed(seed + 100)
        for k in st:
            if k.endswith("running_mean"):
                st[k] = 0.3 * torch.randn(st[k].shape, generator=g)
            elif k.endswith("running_var"):
                st[k] = 0.5 + 1.5 * torch.rand(st[k].shape, generator=g)
    m = STSE(2, [32, 16, 32], 64, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    return m, st


@pytest.mark.parametrize("T,V", GEOMETRIES)
def test_model_eval_on_both_routes(T, V):
    from coskad_amd import engine, ops
    from coskad_amd.models.graph_layers.stsgcn import plan_stack
    x = R.synthetic_clips(5, T=T, V=V, seed=T + V)
    m, st = _stse(T, V)
    m.cuda().eval()
    layers = list(m.encoder.model)
    with torch.no_grad():
        z_ref = R.stse_encode(x, {k: v.clone() for k, v in st.items()}, training=False)
        if (ops.layer_first_pair_ok(2, 32, 16, T, V) and ops.layer_apply_window_ok(T, V, 16, 32)
                and ops.layer_apply_window_ok(T, V, 32, 64)):
            assert plan_stack(layers, False) == [("window_eval", 0, 4)]
        z = m(x.cuda()).cpu()
        np.testing.assert_allclose(z.numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)
        engine.EVAL_WINDOW = False
        try:
            assert plan_stack(layers, False) == [("wide", i, i + 1) for i in range(4)]
            z_composed = m(x.cuda()).cpu()
        finally:
            engine.EVAL_WINDOW = True
        np.testing.assert_allclose(z_composed.numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)


def test_fold_does_not_survive_a_training_step():
    from coskad_amd.trainer import make_train_step
    T, V = 8, 17
    x = R.synthetic_clips(5, T=T, V=V, seed=3)
    m, st = _stse(T, V)
    m.cuda().eval()
    with torch.no_grad():
        z_old = m(x.cuda()).cpu()                           # folds and caches
    np.testing.assert_allclose(z_old.numpy(), R.stse_encode(x, {k: v.clone() for k, v in st.items()}, training=False).numpy(),
                               rtol=1e-4, atol=1e-4)
    m.train()
    eng = make_train_step(m, lr=1e-2, alpha=1e-6, head='euclidean')
    eng.step(x.cuda())
    torch.cuda.synchronize()
    m.eval()
    with torch.no_grad():
        z_new = m(x.cuda()).cpu()
        st_new = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        z_ref = R.stse_encode(x, st_new, training=False)
    assert float((z_ref - z_old).abs().max()) > 1e-2, "the step changed nothing: the test shows nothing"
    np.testing.assert_allclose(z_new.numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)


def test_mixed_decoder_stack():
    from coskad_amd.models.graph_layers.stsgcn import plan_stack
    from coskad_amd.models.sts.ae import STSAE
    T, V, B, hid, L = 8, 17, 4, 64, 8
    st = R.init_stse_state(2, (32, 16, 32), hid, L, T, V, seed=5, decoder=True)
    st["c"] = torch.linspace(-0.2, 0.2, L)
    x = R.synthetic_clips(B, T=T, V=V, seed=6)
    m = STSAE(2, [32, 16, 32], hid, L, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    m.cuda().eval()
    dec = list(m.decoder.model)
    assert [(l.in_channels, l.out_channels) for l in dec] == [(64, 32), (32, 16), (16, 32), (32, 2)]
    with torch.no_grad():
        assert plan_stack(dec, False) == [("wide", 0, 1), ("window_eval", 1, 3), ("wide", 3, 4)]
        assert plan_stack(list(m.encoder.model), False) == [("window_eval", 0, 4)]
        z, xr = m(x.cuda())
        ste = {k: v.clone() for k, v in st.items()}
        z_ref = R.stse_encode(x, ste, training=False)
        xr_ref = R.stsae_decode(z_ref, ste, hid, T, V, training=False)
    np.testing.assert_allclose(z.cpu().numpy(), z_ref.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(xr.cpu().numpy(), xr_ref.numpy(), rtol=1e-4, atol=1e-4)
