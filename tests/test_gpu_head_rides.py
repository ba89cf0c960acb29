"""Work that rides in launches that are there anyway.  The Euclidean head riding in the bottleneck backward's launch
(csrc/btlnk_chain.hip, HD form; engine.HEAD_RIDES) against the separate launches it replaces -- coskad_btlnk_fwd_ws_f32 (partials + their sum), coskad_mse_head_f32 (+ finalize) and
coskad_btlnk_bwd_chain_f32 -- in the same process.  Every comparison is bitwise: the riding form uses the same expressions in the
same order, so a single differing bit is a bug.  The forward operand tables riding in the first layer's moments launch
(engine.FTAB_RIDES) against coskad_build_ftab_f32.  Train steps with both switches on against both off."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, V, HID = 12, 17, 64          # T V = 204 = 12 position tiles of 16 + one of 12


def _inputs(B, Ci, L, seed):
    g = torch.Generator().manual_seed(seed)
    K = HID * T * V
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    return dict(U=r(B, HID, T, V), W=r(L, K, scale=K ** -0.5), b=r(L), c=r(L, scale=0.3), x_in=r(B, Ci, T, V), Z=r(B, Ci, T, V),
                slope=torch.tensor([0.3]).cuda(), in_slope=torch.tensor([0.2]).cuda())


def _same_bits(a, b):
    """bitwise equality (the chain buffer ends in fp64 sums: read as fp32 words, some are NaN patterns, which torch.equal calls unequal)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _grads(L, fill):
    K = HID * T * V
    return (torch.full((L, K), fill, device="cuda"), torch.full((L,), fill, device="cuda"), torch.full((1,), fill, device="cuda"))


def _separate(d, acc, accumulate, grads):
    from coskad_amd import engine, ops
    ws = engine.Workspace()
    z = ops.btlnk_fwd(d["U"], d["W"], d["b"], d["slope"], ws=ws)
    stats, dz, score = ops.mse_head(z, d["c"], need_score=True, acc=acc)
    dW, db, da = grads
    dU, (chain, rows) = ops.btlnk_bwd_chain(d["U"], d["W"], dz, d["slope"], dW, db, da, ws, d["x_in"], d["Z"], d["in_slope"],
                                            accumulate=accumulate)
    return dict(z=z, dz=dz, score=score, stats=stats, dU=dU, chain=chain, rows=rows, dW=dW, db=db, dslope=da)


def _riding(d, acc, accumulate, grads):
    from coskad_amd import engine, ops
    ws = engine.Workspace()
    part = ops.btlnk_fwd_parts(d["U"], d["W"], d["slope"])
    dW, db, da = grads
    z, dz, score, stats, dU, (chain, rows) = ops.btlnk_bwd_chain_head(d["U"], d["W"], part, d["b"], d["c"], d["slope"], dW, db, da, ws,
                                                                      d["x_in"], d["Z"], d["in_slope"], acc=acc, need_score=True,
                                                                      accumulate=accumulate)
    return dict(z=z, dz=dz, score=score, stats=stats, dU=dU, chain=chain, rows=rows, dW=dW, db=db, dslope=da)


# B = 16: the single head block, which writes stats itself; 40: ragged (a last 16-clip tile of 8, chunks ending mid-tile); 600: two head
# blocks, the second partly empty, finished by the reduce launch's extra block.  Ci = 16: the <1> instantiation.
@pytest.mark.parametrize("B,Ci,L", [(16, 32, 16), (40, 32, 16), (600, 32, 16), (16, 32, 8), (40, 32, 8), (600, 32, 8), (40, 16, 16),
                                    (600, 16, 8)])
def test_riding_head_equals_the_separate_launches(B, Ci, L):
    from coskad_amd import ops
    d = _inputs(B, Ci, L, seed=B + Ci + L)
    acc_a = torch.zeros(ops.head_slots(L), device="cuda")
    acc_b = torch.zeros_like(acc_a)
    for call in range(2):                        # acc accumulates over two calls
        want = _separate(d, acc_a, False, _grads(L, float("nan")))
        got = _riding(d, acc_b, False, _grads(L, float("nan")))
        assert got["rows"] == want["rows"] > 0
        for k in ("z", "dz", "score", "stats", "dU", "dW", "db", "dslope", "chain"):
            assert _same_bits(got[k], want[k]), (k, call)
        assert torch.equal(acc_b, acc_a), call
        assert torch.equal(ops.chain_sums(got["chain"], got["rows"], Ci, HID), ops.chain_sums(want["chain"], want["rows"], Ci, HID))
    assert float(acc_a[ops.head_count_slot(L)]) == 2 * B
    want = _separate(d, None, True, _grads(L, 0.25))
    got = _riding(d, None, True, _grads(L, 0.25))
    for k in ("stats", "dU", "dW", "db", "dslope", "chain"):
        assert _same_bits(got[k], want[k]), (k, "accumulate")


def _train(flag, use_graph, B=48):
    """engine.HEAD_RIDES and engine.FTAB_RIDES both `flag`; three STSETrainStep.step calls on clips that differ per step -> (stats per step, state_dict, Adam moments, centre sums).  The
    first graph-mode call takes its step twice (an eager warm-up outside the capture, then the replay), so the eager run repeats its
    first input."""
    from coskad_amd import engine
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import STSETrainStep
    from coskad_amd.utils.synthetic import synthetic_clips
    old = engine.HEAD_RIDES, engine.FTAB_RIDES
    engine.HEAD_RIDES = engine.FTAB_RIDES = flag
    try:
        torch.manual_seed(3)
        model = STSE(2, [32, 16, 32], HID, 16, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0)
        model.c.copy_(torch.linspace(-0.2, 0.2, 16))
        eng = STSETrainStep(model.cuda().train(), lr=1e-3, alpha=1e-6, head='euclidean', use_graph=use_graph)
        xs = [synthetic_clips(B, 2, T, V, seed=10 + i).cuda() for i in range(3)]
        stats = [eng.step(x).clone() for x in (xs if use_graph else xs[:1] + xs)]
        torch.cuda.synchronize()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        return stats[-3:], state, eng.m.clone(), eng.v.clone(), eng.center_acc.clone()
    finally:
        engine.HEAD_RIDES, engine.FTAB_RIDES = old


def _same_run(a, b):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"stats of step {i}"
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), "Adam moments"
    assert torch.equal(a[4], b[4]), "center_acc"


@pytest.fixture(scope="module")
def separate_run():
    return _train(False, False)


def test_train_steps_equal_with_the_head_riding(separate_run):
    got = _train(True, False)
    assert float(got[4][17]) == 4 * 48          # four batches of centre sums
    _same_run(got, separate_run)


def test_captured_step_with_the_head_riding(separate_run):
    """hipGraph capture of the riding form: equal to the captured separate launches, and to the eager step"""
    got = _train(True, True)
    _same_run(got, _train(False, True))
    _same_run(got, separate_run)


@pytest.mark.parametrize("B", [5, 600])
def test_operand_tables_riding_in_the_first_moments_launch(B):
    """engine.FTAB_RIDES: the forward operand tables of the layers above, built by extra blocks of the first layer's moments launch
    (csrc/first_layer.hip), equal coskad_build_ftab_f32's; the moments' partial rows, the stored Z and the fold are unchanged.
    B = 5: one moments block, partly empty; 600: 75 blocks."""
    from coskad_amd import ops
    Ci, Co = 2, 32
    g = torch.Generator().manual_seed(B)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    x = r(B, Ci, T, V)
    A, Tm = r(T, V, V, scale=V ** -0.5), r(V, T, T, scale=T ** -0.5)
    Wt, Wr = r(Co, Ci), r(Co, Ci)
    vec = lambda: r(Co, scale=0.2)
    bt, gt, bet, br, gr, ber = vec(), 1 + vec(), vec(), vec(), 1 + vec(), vec()
    As, Ts = [r(T, V, V) for _ in range(3)], [r(V, T, T) for _ in range(3)]
    E, rows = 2 * (Ci * Ci + Ci), min((B + 7) // 8, 512)

    def run(ride):
        run_stats = [torch.zeros(Co).cuda(), torch.ones(Co).cuda(), torch.zeros((), dtype=torch.int64).cuda(),
                     torch.zeros(Co).cuda(), torch.ones(Co).cuda(), torch.zeros((), dtype=torch.int64).cuda()]
        ws = torch.zeros(ops.train_stats_ws_bytes(Ci), dtype=torch.uint8, device="cuda")
        Z = torch.full_like(x, float("nan"))
        tabs = [torch.full((ops.ftab_floats(),), float("nan"), device="cuda") for _ in range(3)]
        if not ride:
            ops.build_ftabs(As, Ts, tabs)
        out = ops.layer_train_stats(x, A, Tm, None, Wt, bt, gt, bet, *run_stats[:3], Wr, br, gr, ber, *run_stats[3:], ws, Z=Z,
                                    ftabs=(As, Ts, tabs) if ride else None)
        return list(out) + [Z, ws[:rows * E * 4].clone()] + tabs + run_stats

    want, got = run(False), run(True)
    assert not any(bool(torch.isnan(t).any()) for t in got[5:8]), "a table element was not written"
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
