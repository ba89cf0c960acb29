"""Online scoring on the CPU (coskad_amd/stream.py, csrc/stream.hip): the host bookkeeping `StreamPlan` replays the golden test split into
exactly the window table of PoseDatasetRobust and finalises every (person, frame) once; the wrapper's refusals name their reason; the new
entry points refuse bad arguments before they touch a device, and ops.stream_ok restates the library's predicate."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

import stream_refs as SR
from coskad_amd import _lib, ops
from coskad_amd.stream import StreamPlan, StreamScorer
from coskad_amd.utils.argparser import init_sub_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return SR.build_tree(tmp_path_factory.mktemp("morais"), tmp_path_factory.mktemp("exp"))


def _replay(plan, trajs):
    """-> ({track: [first frame of each window]}, [(track, frame id) made final], in the order of emission)"""
    windows, final = {t: [] for t in trajs}, []
    for _, tids in SR.clips_of(trajs).items():
        for f, here, _ in SR.frame_events(trajs, tids):
            p = plan.push(f, here)
            assert len(p.slots) == len(here) and len(set(p.slots)) == len(here)
            assert [i for i in p.out_index if i >= 0] == list(range(len(p.ready_slots)))
            for t, first in zip(p.ready_tracks, p.first_frames):
                windows[t].append(first)
                final.append((t, first))
        for c in plan.close():
            assert len(c.rows) == min(c.count, plan.R - 1)
            final += [(c.track, f) for _, f in c.rows]
        assert plan.live == []
    return windows, final


@pytest.mark.parametrize("seg_len,stride", [(8, 1), (12, 1), (24, 1), (8, 3)])
def test_replay_yields_the_window_table(tree, seg_len, stride):
    from coskad_amd.utils.dataset import PoseDatasetRobust
    root, exp = tree
    ds = PoseDatasetRobust(root, split="test", exp_dir=exp, **dict(SR.BASE, seg_len=seg_len, seg_stride=stride))
    trajs = SR.raw_trajectories(root)
    assert [len(f) for f, _ in trajs.values()] == [33, 12, 18]
    windows, final = _replay(StreamPlan(4, seg_len, stride), trajs)
    rows = [(t[0], t[1], t[2], first) for t in trajs for first in windows[t]]
    assert np.array_equal(np.array(rows, dtype=np.int64).reshape(-1, 4), ds.segs_meta)
    if (seg_len, stride) == (12, 1):
        assert len(rows) == 30
    # every (person, frame id) of the split becomes final exactly once, short tracks included
    want = sorted((t, int(f)) for t, (frames, _) in trajs.items() for f in frames)
    assert sorted(final) == want and len(final) == 63


def test_slots_are_reused_after_close():
    plan = StreamPlan(2, 8)
    a = plan.push(1, ["a", "b"])
    assert a.slots == [0, 1] and a.reset == [1, 1]
    with pytest.raises(ValueError, match="more than max_tracks = 2"):
        plan.push(2, ["a", "b", "c"])
    assert plan.push(2, ["a", "b"]).reset == [0, 0]              # the refused push changed nothing
    closed = plan.close(["a"])
    assert closed[0].slot == 0 and closed[0].count == 2 and closed[0].rows == [(0, 1), (1, 2)]
    c = plan.push(3, ["c", "b"])
    assert c.slots == [0, 1] and c.reset == [1, 0] and plan.count[0] == 1
    with pytest.raises(ValueError, match="not live"):
        plan.close(["a"])


def test_short_track_emits_no_window(tree):
    root, _ = tree
    trajs = SR.raw_trajectories(root, "train")
    tid = next(t for t, (f, _) in trajs.items() if len(f) == 9)
    for seg_len, stride in ((12, 1), (8, 3)):
        plan = StreamPlan(1, seg_len, stride)
        for f in trajs[tid][0]:
            p = plan.push(int(f), [tid])
            assert p.out_index == [-1] and p.ready_tracks == []
        (c,) = plan.close()
        assert c.count == 9 and len(c.rows) == min(9, plan.R - 1) == 9
        assert [f for _, f in c.rows] == [int(f) for f in trajs[tid][0]] and [r for r, _ in c.rows] == list(range(9))
    plan = StreamPlan(1, 8)                                      # R - 1 = 7 < 9: the first two rows are final already
    for f in trajs[tid][0]:
        plan.push(int(f), [tid])
    assert [r for r, _ in plan.close()[0].rows] == list(range(2, 9))


def test_plan_errors_name_their_reason():
    plan = StreamPlan(4, 12)
    with pytest.raises(ValueError, match="duplicate track id 7 in one push"):
        plan.push(1, [7, 3, 7])
    plan.push(5, [7])
    for f in (5, 4):
        with pytest.raises(ValueError, match=f"frame id {f} does not increase within track 7"):
            plan.push(f, [7])
    assert plan.count[0] == 1
    with pytest.raises(ValueError, match="more than max_tracks = 4"):
        plan.push(6, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="unsupported window of 10 frames"):
        StreamPlan(4, 10)
    with pytest.raises(ValueError, match="seg_stride = 0"):
        StreamPlan(4, 12, 0)


def _lit(cls_name, yaml_name, **over):
    from coskad_amd import lit as L
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", yaml_name)), Loader=yaml.FullLoader)
    cfg.update(over)
    args, *_ = init_sub_args(Namespace(**cfg))
    return getattr(L, cls_name)(args)


def test_scorer_refusals_name_their_reason():
    lit = _lit("LitEncoder", "euclidean_encoder.yaml")
    lit.model.train()
    with pytest.raises(ValueError, match="train mode"):
        StreamScorer(lit, None, (1080, 720))
    vae = _lit("LitVAE", "spherical_vae.yaml")
    vae.model.eval()
    with pytest.raises(ValueError, match="LitVAE.*SAMPLED latent"):
        StreamScorer(vae, None, (1080, 720))
    lit3 = _lit("LitEncoder", "euclidean_encoder.yaml", num_coords=3)
    lit3.model.eval()
    with pytest.raises(ValueError, match="num_coords = 3"):
        StreamScorer(lit3, None, (1080, 720))


def test_host_predicate_agrees_with_the_library():
    lib = _lib.lib()
    for T in range(1, 33):
        for V in range(1, 30):
            assert bool(lib.coskad_stream_ok(T, V)) == ops.stream_ok(T, V), (T, V)
    assert [T for T in range(1, 33) if ops.stream_ok(T, 17)] == [8, 12, 16, 24]
    assert [V for V in range(1, 30) if ops.stream_ok(12, V)] == [14, 17, 18]
    assert ops.stream_rows(12, 1) == 12 and ops.stream_rows(8, 3) == 22


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    null = None
    buf = (ctypes.c_double * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    slots = (ctypes.c_int * 4)(0, 1, 2, 3)
    Err = _lib.CoskadHipError

    def push(raw=p, slot=p, slot_host=slots, reset=p, out_index=p, center=p, scale=p, flags=0, mats=p, ring=p, count=p, x_out=p, n=4,
             m=2, M=4, K=5, T=12, V=17, step=1):
        _lib.call("coskad_stream_push_f32", raw, slot, slot_host, reset, out_index, center, scale, 1080.0, 720.0, flags, mats, ring,
                  count, x_out, n, m, M, K, T, V, step, null)

    for name in ("raw", "slot", "slot_host", "reset", "out_index", "mats", "ring", "count", "x_out"):
        with pytest.raises(Err, match=r"\(-1\): stream_push: null pointer"):
            push(**{name: null})
    with pytest.raises(Err, match=r"\(-1\): stream_push: center and scale come together"):
        push(scale=null)
    for kw in (dict(n=0), dict(n=-3), dict(m=5), dict(M=0), dict(K=0), dict(step=0)):
        with pytest.raises(Err, match=r"\(-1\): stream_push: n="):
            push(**kw)
    for kw in (dict(T=10), dict(V=25), dict(T=32), dict(V=16)):
        with pytest.raises(Err, match=r"\(-2\): stream_push: unsupported"):
            push(**kw)
    with pytest.raises(Err, match=r"\(-1\): stream_push: n_joints=18 with layout flags 0"):
        push(V=18)
    for bad in ((0, 1, 2, 4), (0, -1, 2, 3)):
        with pytest.raises(Err, match=r"\(-1\): stream_push: a slot outside \[0, max_tracks\)"):
            push(slot_host=(ctypes.c_int * 4)(*bad))
    with pytest.raises(Err, match=r"\(-1\): stream_push: a slot twice in one launch"):
        push(slot_host=(ctypes.c_int * 4)(0, 1, 1, 3))

    def frames(scores=p, slot=p, slot_host=slots, clip_index=p, count=p, wscore=p, out=p, clip=p, clip_frames=40, m=4, M=4, K=5, T=12,
               step=1):
        _lib.call("coskad_stream_frames_f64", scores, 0, slot, slot_host, clip_index, count, wscore, out, clip, clip_frames, m, M, K, T,
                  step, null)

    for name in ("scores", "slot", "slot_host", "count", "wscore", "out", "clip_index"):
        with pytest.raises(Err, match=r"\(-1\): stream_frames: null pointer"):
            frames(**{name: null})
    for kw in (dict(m=0), dict(K=0), dict(step=-1), dict(clip_frames=0)):
        with pytest.raises(Err, match=r"\(-1\): stream_frames: m="):
            frames(**kw)
    with pytest.raises(Err, match=r"\(-2\): stream_frames: unsupported n_frames=10"):
        frames(T=10)
    with pytest.raises(Err, match=r"\(-1\): stream_frames: a slot outside"):
        frames(M=3)

    def close(row_slot=p, row_slot_host=slots, row_index=p, clip_index=p, count=p, wscore=p, out=p, clip=p, clip_frames=40, rows=4, M=4,
              K=5, T=12, step=1):
        _lib.call("coskad_stream_close_f64", row_slot, row_slot_host, row_index, clip_index, count, wscore, out, clip, clip_frames, rows,
                  M, K, T, step, null)

    for name in ("row_slot", "row_slot_host", "row_index", "count", "wscore", "out", "clip_index"):
        with pytest.raises(Err, match=r"\(-1\): stream_close: null pointer"):
            close(**{name: null})
    with pytest.raises(Err, match=r"\(-1\): stream_close: rows=0"):
        close(rows=0)
    with pytest.raises(Err, match=r"\(-2\): stream_close: unsupported n_frames=10"):
        close(T=10)
    with pytest.raises(Err, match=r"\(-1\): stream_close: a slot outside"):
        close(M=2)


def test_wrappers_have_no_cpu_fallback():
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.stream_push(torch.zeros(1, 34), i32(1), i32(1), i32(1), i32(1), None, None, (1080, 720), 0, torch.zeros(1, 3, 3),
                        torch.zeros(2, 12, 2, 17), i32(2), 0, 12, 17, 1)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.stream_frames(torch.zeros(1), i32(1), i32(1), None, i32(2), torch.zeros(2, 1, 12, dtype=torch.float64), None, 12, 1)
