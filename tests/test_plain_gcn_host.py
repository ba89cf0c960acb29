"""CPU checks of the plain-GCN encoders on the flat train step (coskad_amd.trainer._PlainGCNStack): routing, segment kinds, the
flat buffers' layout, the shape predicate and the new entry points' argument checks.  Construction only: no kernel runs (the built
library is needed for the predicate and the argument checks, as in test_lib_abi.py)."""
import ctypes

import pytest
import torch

from coskad_amd import _lib, ops, trainer
from coskad_amd.models.sts.ae import STSE


def _stse(encoder, projector='linear', widths=(32, 16, 32), hidden=64, latent=16, V=17):
    torch.manual_seed(0)
    return STSE(2, list(widths), hidden, latent, 12, V, encoder, projector, 'euclidean', 0.0).train()


@pytest.mark.parametrize("encoder", ["learnable_gcn", "static_gcn"])
@pytest.mark.parametrize("projector", ["linear", "mlp"])
def test_flat_plain_gcn_step_layout(encoder, projector):
    m = _stse(encoder, projector)
    eng = trainer.make_train_step(m, flat_plain_gcn=True, lr=1e-4, alpha=1e-6)
    assert type(eng) is trainer.STSETrainStep
    segs = eng.stack.segs
    assert len(segs) == len(m.encoder.gcns) == 4
    assert all(s.kind == 'plain' and s[0] == 'plain' and s.out_slope_grad is None and s.fused for s in segs)
    assert eng.stack.last_slope_grad is None and eng.stack.top([None] * 4) == (None, None)
    fp = eng.fp
    first_btlnk = next(n for n in fp.names if n.startswith("btlnk."))
    assert eng.tail_off == fp.offsets[first_btlnk]
    assert all(n.startswith("btlnk.") for n in fp.names[fp.names.index(first_btlnk):])
    # regulariser mask: calc_reg_loss takes every tensor whose name has no 'bias' -- Adj and weight, not bias
    for n in fp.names:
        off, k = fp.offsets[n], fp.views[n].numel()
        want = 0.0 if 'bias' in n else 1.0
        assert bool((fp.reg_mask[off:off + k] == want).all()), n
    adj_names = [n for n in fp.names if n.endswith(".Adj")]
    if encoder == "learnable_gcn":
        assert len(adj_names) == 4 and all(s.gAdj is not None and s.adj is None for s in segs)
    else:
        # the static graph is a buffer: not in the flat buffer, no gradient view
        assert adj_names == [] and all(s.gAdj is None and s.adj is m.encoder.Adj for s in segs)
        assert "encoder.Adj" in m.state_dict() and "encoder.Adj" not in fp.views
    # gradients land in the flat buffer's views
    for i, s in enumerate(segs):
        assert s.gW.data_ptr() == fp.gviews[f"encoder.gcns.{i}.gcn.weight"].data_ptr()
        assert s.gb.data_ptr() == fp.gviews[f"encoder.gcns.{i}.gcn.bias"].data_ptr()


def test_default_routing_is_unchanged():
    for encoder in ("learnable_gcn", "static_gcn"):
        assert type(trainer.make_train_step(_stse(encoder), lr=1e-4)) is trainer.AutogradTrainStep
        assert type(trainer.make_train_step(_stse(encoder), flat_plain_gcn=False, lr=1e-4)) is trainer.AutogradTrainStep
    # the keyword changes nothing for the STS-GCN encoder, and a projector beyond the kernels stays on the autograd step
    assert type(trainer.make_train_step(_stse("sts_gcn"), flat_plain_gcn=True, lr=1e-4)) is trainer.STSETrainStep
    wide_mlp = STSE(2, [8, 4], 8, 128, 12, 17, "learnable_gcn", "mlp", 'euclidean', 0.0, projector_hidden_layers=[128]).train()
    assert not wide_mlp.btlnk.hip_ok
    assert type(trainer.make_train_step(wide_mlp, flat_plain_gcn=True, lr=1e-4)) is trainer.AutogradTrainStep


def test_flat_plain_gcn_step_runs_eagerly_on_the_main_stream():
    """use_graph / side_stream are dropped by make_train_step and refused by the constructor, as for wide stacks"""
    eng = trainer.make_train_step(_stse("learnable_gcn"), flat_plain_gcn=True, lr=1e-4, use_graph=True, side_stream=True, sync_bn=True)
    assert type(eng) is trainer.STSETrainStep and not eng.use_graph and eng.side is None and eng.sync_group is None
    for kw in (dict(use_graph=True), dict(side_stream=True)):
        with pytest.raises(ValueError, match="main stream"):
            trainer.STSETrainStep(_stse("static_gcn"), lr=0.0, **kw)


def test_shapes_outside_the_kernels_stay_in_the_segment():
    """another window length: the same 'plain' segments, on the GEMM composition"""
    m = STSE(2, [8, 4], 8, 8, 8, 17, "learnable_gcn", "linear", 'euclidean', 0.0).train()
    eng = trainer.make_train_step(m, flat_plain_gcn=True, lr=0.0)
    assert [s.kind for s in eng.stack.segs] == ['plain'] * 3 and not any(s.fused for s in eng.stack.segs)


def test_plain_gcn_ok_agrees_with_the_library():
    fn = _lib.lib().coskad_plain_gcn_ok
    fn.restype = ctypes.c_int
    for Ci in (1, 2, 4, 8, 16, 32, 64, 65):
        for Co in (1, 2, 4, 8, 16, 32, 64, 65):
            for P in (136, 168, 204, 216, 300, 408):
                assert ops.plain_gcn_ok(Ci, Co, P) == bool(fn(Ci, Co, P)), (Ci, Co, P)
    assert ops.plain_gcn_ok(2, 32, 204) and ops.plain_gcn_ok(64, 64, 300)
    assert not ops.plain_gcn_ok(65, 8, 204) and not ops.plain_gcn_ok(8, 8, 136) and not ops.plain_gcn_ok(0, 8, 204)


def test_argument_errors_are_reported_without_a_gpu():
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 68)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)       # the activations' 16-byte alignment is checked as well
    i32, sz = _lib.i32, ctypes.c_size_t
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        _lib.call("coskad_plain_gcn_fwd_f32", null, p, p, null, p, null, i32(4), i32(2), i32(8), i32(204), i32(0), null)
    with pytest.raises(_lib.CoskadHipError, match="unsupported"):
        _lib.call("coskad_plain_gcn_fwd_f32", p, p, p, null, p, null, i32(4), i32(2), i32(8), i32(136), i32(0), null)
    with pytest.raises(_lib.CoskadHipError, match="unsupported"):
        _lib.call("coskad_plain_gcn_fwd_f32", p, p, p, null, p, null, i32(4), i32(65), i32(8), i32(204), i32(0), null)
    bwd = lambda *a: _lib.call("coskad_plain_gcn_bwd_f32", *a)
    tail = (i32(4), i32(2), i32(8), i32(204), i32(1), i32(0), i32(0), i32(0), null)
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        bwd(p, p, p, null, p, p, p, p, p, null, p, sz(1 << 20), *tail)                     # dO
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        bwd(p, null, p, p, p, p, p, p, p, null, p, sz(1 << 20), *tail)                     # Ci <= Co needs the saved Y
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        bwd(p, p, p, p, p, p, null, p, p, null, p, sz(1 << 20), *tail)                     # need_dx without dX
    with pytest.raises(_lib.CoskadHipError, match="unsupported"):
        bwd(p, p, p, p, p, p, p, p, p, null, p, sz(1 << 20), i32(4), i32(2), i32(8), i32(408), i32(1), i32(0), i32(0), i32(0), null)
    with pytest.raises(_lib.CoskadHipError, match="workspace"):
        bwd(p, p, p, p, p, p, p, p, p, null, p, sz(8), *tail)
    ws = _lib.lib().coskad_plain_gcn_ws_bytes
    ws.restype = ctypes.c_size_t
    # one partial row [Ci * Co + Co] per workgroup; 4 clips of 2 channels are one group of 16
    assert ws(4, 2, 8, 204, 0) == 1 * (2 * 8 + 8) * 4
    assert ws(37, 2, 8, 204, 2) == 2 * (2 * 8 + 8) * 4
    assert ws(4, 2, 8, 136, 0) == 0
