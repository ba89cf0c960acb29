"""The eval-mode caches (per-layer BatchNorm folds, the fused encoder's operand streams, the folded rev_btlnk + first decoder layer
images) follow training that never goes through `model.train()`: a flat step driven with the module left in eval mode, eagerly or as
a hipGraph replay, writes parameters and running statistics through raw pointers, and the next eval forward must see them
(coskad_amd/ops.py: note_raw_write / raw_write_epoch).  The reference in every case is a newly constructed model (no caches) that
loads the trained model's state; both sides run the same kernels on the same values, so the comparison is torch.equal."""
import pytest
import torch

from conftest import state_from
from test_eval_cache_host import WRITERS, Counter, writer_moves_epoch
from test_gpu_ae_step import _build
from test_gpu_modules import build_stse

pytestmark = pytest.mark.gpu

SMALL = (2, [8, 4, 8], 8, 8, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0)
DEFAULT16 = (2, [32, 16, 32], 64, 16, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0)


def _fresh(m, make):
    """a new model (no cache of any kind) with the state of `m`"""
    ref = make()
    ref.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    return ref.cuda().eval()


def _encode(m, x):
    with torch.no_grad():
        return m(x).clone()


def test_encoder_left_in_eval_mode_eager_step():
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import STSETrainStep
    from oracle import ref_cpu as R
    torch.manual_seed(3)
    m = STSE(*SMALL).cuda().eval()
    x = R.synthetic_clips(6, seed=5).cuda()
    z0 = _encode(m, x)
    eng = STSETrainStep(m, lr=1e-2, alpha=1e-4, head='euclidean')
    for _ in range(2):
        eng.step(x)
    assert not m.training
    z1 = _encode(m, x)
    assert not torch.equal(z1, z0)
    assert torch.equal(z1, _encode(_fresh(m, lambda: STSE(*SMALL)), x))


def test_encoder_left_in_eval_mode_graph_replay(golden):
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import STSETrainStep
    from oracle import ref_cpu as R
    m = STSE(*DEFAULT16)
    m.load_state_dict(state_from(golden("stse_default.npz")), strict=True)
    m.c.fill_(0.05)
    m.cuda().eval()
    xs = [R.synthetic_clips(64, seed=20 + i).cuda() for i in range(3)]
    eng = STSETrainStep(m, lr=1e-2, alpha=1e-4, head='euclidean', use_graph=True)
    z0 = _encode(m, xs[0])
    eng.step(xs[0])                                 # warm-up, capture, replay
    eng.step(xs[1])                                 # replay
    z2 = _encode(m, xs[0])                          # the caches exist when the last replay runs
    assert not torch.equal(z2, z0)
    eng.step(xs[2])                                 # replay: none of the wrappers' Python runs
    torch.cuda.synchronize()
    assert not m.training
    z3 = _encode(m, xs[0])
    assert not torch.equal(z3, z2)
    assert torch.equal(z3, _encode(_fresh(m, lambda: STSE(*DEFAULT16)), xs[0]))


@pytest.mark.parametrize("mode_at_build", ["always", "never"])
def test_decoder_folds_follow_a_step_in_eval_mode(golden, monkeypatch, mode_at_build):
    """the lowrank first decoder layer, a commuted encoder layer and the decoder tail of stsae_v25; `never`: the step object is built
    without the lowrank first layer (so its forward never touches that layer's folded images) and eval mode folds them afterwards"""
    from coskad_amd import lowrank
    from coskad_amd.models.sts.ae import STSAE
    from coskad_amd.trainer import STSAETrainStep
    g = golden("stsae_v25.npz")
    m, st = _build(g, STSAE)
    m.load_state_dict(st, strict=True)
    m.cuda().eval()
    x = torch.from_numpy(g["x"]).cuda()
    assert lowrank.MODE == "always"
    with monkeypatch.context() as mp:
        mp.setattr(lowrank, "MODE", mode_at_build)
        eng = STSAETrainStep(m, mode='ae', lr=1e-2, alpha=0.0, lambda_=1.0)

    def both(model):
        with torch.no_grad():
            return model(x)[1].clone(), model.reconstruction_scores(x)[1].clone()
    r0, s0 = both(m)
    assert "_lowrank_eval" in m.decoder.model[0].__dict__ and m.decoder.model[-1].__dict__["_fold_cache"]
    eng.step(x)
    assert not m.training
    r1, s1 = both(m)
    assert not torch.equal(r1, r0) and not torch.equal(s1, s0)
    rr, sr = both(_fresh(m, lambda: _build(g, STSAE)[0]))
    assert torch.equal(r1, rr)
    assert torch.equal(s1, sr)


@pytest.mark.parametrize("name", ["stse_default.npz", "stse_v25.npz", "stsae_v25.npz"])
def test_steady_state_eval_stays_cached(golden, monkeypatch, name):
    """stse_default: the fused plan; stse_v25: per-layer folds; stsae_v25: those, the folded first decoder layer and the tail"""
    from coskad_amd import lowrank, ops
    from coskad_amd.models.sts.ae import STSAE
    g = golden(name)
    if name.startswith("stsae"):
        m, st = _build(g, STSAE)
        m.load_state_dict(st, strict=True)
        m.cuda()
    else:
        m, _ = build_stse(g)
    m.eval()
    x = torch.from_numpy(g["x"]).cuda()
    counters = [Counter(ops.bn_fold), Counter(ops.gather), Counter(lowrank.fold_eval)]
    monkeypatch.setattr(ops, "bn_fold", counters[0])
    monkeypatch.setattr(ops, "gather", counters[1])
    monkeypatch.setattr(lowrank, "fold_eval", counters[2])

    def forward():
        with torch.no_grad():
            m(x)
            if isinstance(m, STSAE):
                m.reconstruction_scores(x)
    forward()
    first = [c.n for c in counters]
    assert sum(first) > 0
    if name == "stse_default.npz":
        assert "_fused_plan" in m.__dict__ and first[1] == 3
    if isinstance(m, STSAE):
        assert first[2] == 1
    forward()
    forward()
    assert [c.n for c in counters] == first


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_writer_moves_epoch(name, monkeypatch):
    """every wrapper that hands the library module state to write moves the epoch (the library calls are no-ops here)"""
    assert writer_moves_epoch(name, "cuda", monkeypatch)


def test_eval_mode_statistics_leave_the_epoch(monkeypatch):
    """bn2_stats and mlp_head_fwd write nothing in eval mode: a bump there would refold every model on every eval forward"""
    from coskad_amd import ops
    monkeypatch.setattr(ops, "call", lambda *a, **k: None)
    dev = torch.device("cuda")
    f = lambda *s: torch.zeros(*s, device=dev)
    before = ops.raw_write_epoch()
    ops.bn2_stats(f(2, 16, 204), torch.nn.BatchNorm2d(16).to(dev), False)
    ops.mlp_head_fwd(f(2, 32), f(32), f(32), f(32), f(32), torch.zeros((), dtype=torch.int64, device=dev), f(8, 32), f(8), False)
    assert ops.raw_write_epoch() == before
