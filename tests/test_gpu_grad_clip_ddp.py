"""Two ranks on ONE GPU over gloo (as tests/test_gpu_ddp.py): accumulate = 2 with norm clipping.  No collective inside an
accumulation group, one all-reduce of the accumulated buffer per update, clipping after it: both ranks end with the parameters
and Adam moments of the torch yardstick, each update over four micro-batches (loss / 4, each with its own BatchNorm batch
statistics).  Two updates: after one update from zero moments the parameters move by lr * sign(g) whatever the clip coefficient
and the 1 / (world * k), so the first is held by the norm and the moments and only the second by the parameters."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_ddp import _free_port
from test_gpu_grad_clip_step import ALPHA, LR, ZERO_GRAD, Yardstick, _stse, clips, compared, flat_moments, grad_tol

pytestmark = pytest.mark.gpu
MICRO = 6           # clips per micro-batch: in update u rank r takes micro-batches 4 u + 2 r and 4 u + 2 r + 1 of the 48 clips


def _worker(rank, world, port, q, clip):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from coskad_amd.trainer import STSETrainStep
    calls, real = [], dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    dist.all_reduce = counted
    m = _stse()
    eng = STSETrainStep(m, lr=LR, alpha=ALPHA, head='euclidean', grad_clip_val=clip, accumulate=2)
    assert eng.world == world
    seen, norms, first = [], [], None
    for u in range(2):
        for i in range(2):
            lo = (4 * u + 2 * rank + i) * MICRO
            eng.step(clips(lo, lo + MICRO))
            seen.append(len(calls))
        norms.append(float(eng.last_grad_norm))
        if u == 0:
            first = (flat_moments(eng, eng.m), flat_moments(eng, eng.v))
    torch.cuda.synchronize()
    dist.all_reduce = real
    q.put((rank, {k: v.detach().cpu().numpy() for k, v in m.named_parameters()}, seen, eng.updates, norms, first,
           (flat_moments(eng, eng.m), flat_moments(eng, eng.v))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate_and_clip():
    world = 2
    yard = Yardstick()
    for i in range(4):
        yard.backward(clips(i * MICRO, (i + 1) * MICRO), 0.25)
    clip = yard.update(frac=0.01)
    ref_norms = [yard.norm]
    ref_first = (yard.moments('exp_avg'), yard.moments('exp_avg_sq'))
    for i in range(4, 8):
        yard.backward(clips(i * MICRO, (i + 1) * MICRO), 0.25)
    yard.update(clip)
    ref_norms.append(yard.norm)
    ref_last = (yard.moments('exp_avg'), yard.moments('exp_avg_sq'))
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, clip)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    ref = {n: p.detach().cpu().numpy() for n, p in yard.m.named_parameters()}
    for rank, got, seen, updates, norms, first, last in res:
        assert seen == [0, 1, 1, 2] and updates == 2    # collectives == updates: none on the micro-step inside a group
        np.testing.assert_allclose(norms, ref_norms, rtol=2e-3)
        for mom, ref_mom in ((first, ref_first), (last, ref_last)):
            for g, r, rtol in zip(mom, ref_mom, (2e-3, 4e-3)):      # exp_avg, exp_avg_sq at the gradient tolerance
                for n, (rt, at) in grad_tol(r, compared(r), rtol).items():
                    np.testing.assert_allclose(g[n], r[n], rtol=rt, atol=at, err_msg=f"rank {rank} {n}")
        for n in ref:
            if not n.endswith(ZERO_GRAD):
                np.testing.assert_allclose(got[n], ref[n], rtol=2e-3, atol=2e-5, err_msg=f"rank {rank} {n}")
    for n in ref:
        np.testing.assert_array_equal(res[0][1][n], res[1][1][n], err_msg=n)
