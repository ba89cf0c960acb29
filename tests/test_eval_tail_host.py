"""CPU checks of the decoder-tail kernel (csrc/eval_tail_window.hip): the set its predicate states, that the other
predicates keep their answers for two output channels, what the C ABI says before it touches a device, and the CPU fallbacks of
STSAE.reconstruction_scores and eval_utils.rec_and_hy_from_rec.  No kernel runs."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops
from coskad_amd.models.sts.ae import STSAE
from coskad_amd.utils import eval_utils

SUPPORTED = {(T, V, Ci, 2) for T in (8, 12, 16, 24) for V in (17, 25) for Ci in (16, 32)}


def test_predicate_is_the_stated_set():
    fn, grid = _lib.lib().coskad_layer_tail_ok, _lib.lib().coskad_layer_tail_max_grid
    seen = set()
    for T in (4, 8, 10, 12, 16, 20, 24, 32):
        for V in (14, 17, 18, 25, 26):
            for Ci in (2, 8, 16, 32, 64):
                for Co in (1, 2, 3, 4, 16):
                    got = fn(T, V, Ci, Co)
                    assert got in (0, 1)
                    assert bool(got) == ((T, V, Ci, Co) in SUPPORTED), (T, V, Ci, Co)
                    assert ops.layer_tail_ok(T, V, Ci, Co) == (bool(got) and (T, V) not in ops.LAYER_TAIL_OFF)
                    seen.add((T, V, Ci, Co)) if got else None
                assert (grid(T, V, Ci) > 0) == ((T, V, Ci, 2) in SUPPORTED), (T, V, Ci)
    assert seen == SUPPORTED and len(SUPPORTED) == 16


def test_switch_off_table_is_honoured(monkeypatch):
    assert isinstance(ops.LAYER_TAIL_OFF, frozenset)
    monkeypatch.setattr(ops, "LAYER_TAIL_OFF", frozenset({(16, 25)}))
    assert not ops.layer_tail_ok(16, 25, 32, 2) and ops.layer_tail_ok(16, 17, 32, 2) and ops.layer_tail_ok(8, 25, 32, 2)
    assert _lib.lib().coskad_layer_tail_ok(16, 25, 32, 2) == 1      # the library states what is built, the table what is used


def test_existing_predicates_keep_their_answers():
    lib = _lib.lib()
    for T in (8, 12, 16, 24):
        for V in (17, 25):
            for Ci in (16, 32):
                assert lib.coskad_layer_tail_ok(T, V, Ci, 2) == 1         # the tail's set is its own: where it holds, the others ..
                assert lib.coskad_layer_apply_window_ok(T, V, Ci, 2) == 0
                assert lib.coskad_layer_train_window_ok(T, V, Ci, 2) == 0
                assert lib.coskad_layer_train_window_narrow_ok(T, V, Ci, 2) == 0
                assert lib.coskad_layer_first_pair_ok(T, V, Ci, 32, 2) == 0
    for T, V in ((8, 17), (24, 25)):
        assert lib.coskad_layer_apply_window_ok(T, V, 32, 32) == 1
        assert lib.coskad_layer_train_window_narrow_ok(T, V, 4, 2) == 1
    from coskad_amd.models.graph_layers.stsgcn import layer_fits
    for T, V in ((12, 17), (12, 25), (8, 17)):
        assert bool(lib.coskad_layer_fits(32, 2, T, V)) == layer_fits(32, 2, T, V)


def _aligned(n_floats):
    """a host buffer and a 16-byte aligned address inside it"""
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_argument_checks_come_before_the_device():
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    odd = ctypes.c_void_p(a + 4)

    def tail(inp=p, x=p, out=p, score=p, A=p, wfold=p, B=1, T=8, V=17, Ci=32, Co=2):
        _lib.call("coskad_layer_tail_f32", inp, x, out, score, A, p, wfold, p, null, null, B, Ci, Co, T, V, null)

    for kw in (dict(inp=null), dict(A=null), dict(wfold=null)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*null pointer"):
            tail(**kw)
    for B in (0, -3):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*B=" + str(B)):
            tail(B=B)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`in`.*16-byte aligned"):
        tail(inp=odd)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`x`.*16-byte aligned"):
        tail(x=odd)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`out`.*16-byte aligned"):
        tail(out=odd)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`in`.*16-byte aligned"):
        tail(inp=odd, V=14)                                # the pointer is judged before the shape
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*neither"):
        tail(out=null, score=null)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`score` needs"):
        tail(x=null)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`score` needs"):
        tail(x=null, out=null)
    for kw in (dict(T=11), dict(V=14), dict(Ci=8), dict(Co=3)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\): unsupported"):
            tail(**kw)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\): unsupported"):
        tail(x=null, score=null, Co=3)                     # out alone is a complete call: the shape is what is wrong


def _cpu_model(T=8, V=17):
    from oracle import ref_cpu as R
    st = R.init_stse_state(2, (32, 16, 32), 64, 8, T, V, seed=4, decoder=True)
    st["c"] = torch.linspace(-0.2, 0.2, 8)
    m = STSAE(2, [32, 16, 32], 64, 8, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
    m.load_state_dict(st, strict=True)
    return m.eval()


def test_reconstruction_scores_on_cpu_tensors_is_the_formula_on_forward(monkeypatch):
    m = _cpu_model()
    assert m._tail_layer(torch.zeros(1)) is None            # a CPU tensor never reaches the kernel
    x = torch.randn(3, 2, 8, 17)
    z, x_rec = torch.randn(3, 8), torch.randn(3, 2, 8, 17)
    monkeypatch.setattr(STSAE, "forward", lambda self, X: (z, x_rec))
    with torch.no_grad():
        got_z, rec = m.reconstruction_scores(x)
    assert got_z is z and rec.shape == (3,)
    assert torch.equal(rec, ((x_rec - x) ** 2).reshape(3, -1).mean(-1))


def test_rec_and_hy_from_rec_agrees_with_the_window_scores():
    g = torch.Generator().manual_seed(0)
    x, x_rec = torch.randn(6, 2, 8, 17, generator=g), torch.randn(6, 2, 8, 17, generator=g)
    z, c = torch.randn(6, 8, generator=g), torch.randn(8, generator=g)
    rec = ((x_rec - x) ** 2).reshape(6, -1).mean(-1)
    for kind in ('rec', 'hyp', 'rec+hyp'):
        want = eval_utils.rec_and_hy_window_scores(x, x_rec, z, c, 0.2, kind)
        assert torch.equal(eval_utils.rec_and_hy_from_rec(rec, z, c, 0.2, kind), want), kind
    assert torch.equal(eval_utils.rec_and_hy_from_rec(None, z, c, 0.2, 'hyp'), ((z - c) ** 2).mean(-1))
    with pytest.raises(ValueError):
        eval_utils.rec_and_hy_from_rec(rec, z, c, 0.2, 'other')
