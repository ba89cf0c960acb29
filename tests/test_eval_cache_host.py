"""CPU checks of the one rule that keeps the eval-mode caches fresh (coskad_amd/ops.py: note_raw_write / raw_write_epoch): every cache
key carries the raw-write epoch beside the (data_ptr, _version) pairs, and every wrapper that hands the library module state to write
moves the epoch.  CPU tensors and counting torch stand-ins for ops.bn_fold / ops.gather: no native library, no kernel."""
import pytest
import torch
from torch import nn

from coskad_amd import _lib, engine, ops
from coskad_amd.models.graph_layers.stsgcn import layer_tensors
from coskad_amd.models.sts.ae import STSE


class Counter:
    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **k):
        self.n += 1
        return self.fn(*a, **k)


def _bn_fold(Wt, *rest):
    Co, Ci = Wt.shape
    return torch.zeros(2 * Ci, ops.cop(Co)), torch.zeros(ops.cop(Co))


def _gather(src, idx):
    return torch.zeros(idx.shape)


@pytest.fixture
def counted(monkeypatch):
    """ops.bn_fold and ops.gather replaced by counting stand-ins -> (folds, gathers)"""
    folds, gathers = Counter(_bn_fold), Counter(_gather)
    monkeypatch.setattr(ops, "bn_fold", folds)
    monkeypatch.setattr(ops, "gather", gathers)
    return folds, gathers


def _encoder(V=17):
    torch.manual_seed(0)
    return STSE(2, [32, 16, 32], 64, 8, 12, V, 'sts_gcn', 'linear', 'euclidean', 0.0).eval()


def test_eval_fold_follows_epoch_and_versions(counted):
    folds, _ = counted
    m = _encoder()
    L = layer_tensors(m.encoder.model[1])
    first = engine.eval_fold(L)
    assert engine.eval_fold(L) is first and folds.n == 1            # two calls in a row: one fold
    ops.note_raw_write()
    second = engine.eval_fold(L)
    assert folds.n == 2 and second is not first                     # a raw write somewhere: folded again
    assert engine.eval_fold(L) is second and folds.n == 2
    with torch.no_grad():
        m.encoder.model[1].tcn[1].running_var.mul_(1.5)             # a torch-side write: the version counter moves
    engine.eval_fold(L)
    assert folds.n == 3
    engine.eval_fold(layer_tensors(m.encoder.model[1]))             # fresh views of the same layer share the layer's cache
    assert folds.n == 3


def test_eval_fold_without_a_cache_folds_every_time(counted):
    folds, _ = counted
    L = layer_tensors(_encoder().encoder.model[0])
    L.cache = None
    engine.eval_fold(L)
    engine.eval_fold(L)
    assert folds.n == 2


def test_fused_plan_follows_epoch_and_versions(counted):
    folds, gathers = counted
    m = _encoder(17)
    layers = [layer_tensors(l) for l in m.encoder.model]
    assert engine.fused_encoder_supported(layers, 12, 17)
    plan = engine.FusedEncoderPlan()
    W = (m.btlnk.weight,)
    assert plan.get(layers, W) is plan
    assert (folds.n, gathers.n) == (4, 3)                            # one fold per layer, one gather per operand stream
    tab = plan.tab
    assert plan.get(layers, W) is plan and plan.tab is tab and (folds.n, gathers.n) == (4, 3)      # unchanged inputs: no rebuild
    ops.note_raw_write()
    plan.get(layers, W)
    assert (folds.n, gathers.n) == (8, 6) and plan.tab is not tab    # a raw write: everything again
    assert plan.get(layers, W) is plan and (folds.n, gathers.n) == (8, 6)
    with torch.no_grad():
        m.btlnk.weight.mul_(2.0)                                     # the bottleneck weight changed in place: the streams again
    plan.get(layers, W)
    assert gathers.n == 9
    assert not hasattr(plan, "token") and all("fused" not in L.cache for L in layers)


# ---- every writer moves the epoch --------------------------------------------------------------------------------------------------
B, CI, CO, T, V = 2, 16, 16, 12, 17


def _bn(dev, C=CO):
    return nn.BatchNorm2d(C).to(dev)


def _layer_args(dev, Ci=CI, Co=CO):
    """Wt, bt, gt, bet, rm_t, rv_t, nbt_t, Wr, br, gr, ber, rm_r, rv_r, nbt_r of a (Ci -> Co) layer"""
    f = lambda *s: torch.zeros(*s, device=dev)
    half = lambda: [f(Co, Ci), f(Co), f(Co), f(Co), f(Co), f(Co), torch.zeros((), dtype=torch.int64, device=dev)]
    return half() + half()


def _ws(dev, nbytes):
    return torch.empty(nbytes() if dev.type == "cuda" else 1024, dtype=torch.uint8, device=dev)


def _train_stats(dev):
    f = lambda *s: torch.zeros(*s, device=dev)
    ops.layer_train_stats(f(B, CI, T, V), f(T, V, V), f(V, T, T), None, *_layer_args(dev), _ws(dev, lambda: ops.train_stats_ws_bytes(CI)))


def _train_fold(dev):
    ops.layer_train_fold(torch.zeros(4 * 2 * (CI * CI + CI), device=dev), 4, B, T, V, *_layer_args(dev),
                         _ws(dev, lambda: ops.train_stats_ws_bytes(CI)))


def _train_fold_sums(dev):
    ops.layer_train_fold_sums(torch.zeros(2 * (CI * CI + CI), device=dev, dtype=torch.float64), float(B * T * V), *_layer_args(dev))


def _commute(dev):
    f = lambda *s: torch.zeros(*s, device=dev)
    v = lambda: f(16)
    nbt = lambda: torch.zeros((), dtype=torch.int64, device=dev)
    ops.commute_fwd(f(B, 32, T, 25), None, f(16, 32), f(16, 32), f(T, 25, 25), f(25, T, T), v(), v(), v(), v(), None, None, v(), v(), v(),
                    v(), nbt(), nbt(), 0.1, 1e-5)


def _bn2_stats(dev):
    ops.bn2_stats(torch.zeros(B, CO, T * V, device=dev), _bn(dev), True)


def _bn2_stats_parts(dev):
    ops.bn2_stats_parts(torch.zeros(3, CO, 2, device=dev, dtype=torch.float64), _bn(dev), B * T * V)


def _mlp_head(dev):
    f = lambda *s: torch.zeros(*s, device=dev)
    ops.mlp_head_fwd(f(B, 32), f(32), f(32), f(32), f(32), torch.zeros((), dtype=torch.int64, device=dev), f(8, 32), f(8), True)


def _lowrank_fold(dev):
    ops.lowrank_fold_fwd(torch.zeros(2, 9, CO, T * V, device=dev), torch.zeros(9, 9, device=dev, dtype=torch.float64), _bn(dev), _bn(dev),
                         None, None, float(B * T * V))


def _adam_args(dev):
    return [torch.zeros(64, device=dev) for _ in range(4)] + [None]


def _adam(dev):
    ops.adam(*_adam_args(dev), 1e-3, 0.9, 0.999, 1e-8, 1)


def _adam_pow(dev):
    ops.adam_pow(*_adam_args(dev), 1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999)


def _adam_dev(dev):
    ops.adam_dev(*_adam_args(dev), torch.zeros(4, device=dev), 0.9, 0.999, 1e-8)


# the wrappers whose entry points take module state through non-const pointers (include/coskad_hip.h)
WRITERS = {"layer_train_stats": _train_stats, "layer_train_fold": _train_fold, "layer_train_fold_sums": _train_fold_sums,
           "commute_fwd": _commute, "bn2_stats": _bn2_stats, "bn2_stats_parts": _bn2_stats_parts, "mlp_head_fwd": _mlp_head,
           "lowrank_fold_fwd": _lowrank_fold, "adam": _adam, "adam_pow": _adam_pow, "adam_dev": _adam_dev}


def writer_moves_epoch(name, dev, monkeypatch) -> bool:
    """run the wrapper with zero tensors on `dev` and every library call a no-op: did the epoch move?"""
    monkeypatch.setattr(ops, "call", lambda *a, **k: None)
    before = ops.raw_write_epoch()
    WRITERS[name](torch.device(dev))
    return ops.raw_write_epoch() > before


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_writer_moves_epoch(name, monkeypatch):
    monkeypatch.setattr(ops, "_stream", lambda: None)
    try:
        moved = writer_moves_epoch(name, "cpu", monkeypatch)
    except _lib.CoskadHipError as e:
        assert "expected a CUDA (ROCm) tensor" in str(e)
        pytest.skip(f"ops.{name} checks is_cuda before anything else: tests/test_gpu_eval_cache.py::test_writer_moves_epoch covers it")
    assert moved
