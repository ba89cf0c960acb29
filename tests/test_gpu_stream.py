"""Online scoring on the GPU (coskad_amd/stream.py, csrc/stream.hip): the golden test split replayed frame by frame must give the offline
route's windows, window scores, person-frame means and clip vectors bit for bit; the frames launch against a float64 numpy restatement on
hand-made scores; a push never synchronises; stream_COSKAD.py prints eval_COSKAD.py's AUC."""
import glob
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

import stream_refs as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"plain": {}, "kp18": dict(kp18_format=True), "headless": dict(headless=True)}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return SR.build_tree(tmp_path_factory.mktemp("morais"), tmp_path_factory.mktemp("exp"))


def _dataset(tree, **over):
    from coskad_amd.utils.dataset import PoseDatasetRobust
    root, exp = tree
    return PoseDatasetRobust(root, split="test", exp_dir=exp, **dict(SR.BASE, **over))


def _window_of(ds):
    """{(scene, clip, person, first frame): window index}"""
    return {tuple(int(v) for v in r): s for s, r in enumerate(ds.segs_meta)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 3. windows ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seg_len,stride", [(8, 1), (12, 1), (24, 1), (8, 3)])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_streamed_windows_are_the_dataset_items(tree, layout, seg_len, stride):
    """kernel level: the plan's tables and coskad_stream_push_f32 alone, K = 5.  The 33-row track wraps a ring of 12 rows more than
    twice; stride 3 at 8 frames is a ring of 22."""
    from coskad_amd import ops
    from coskad_amd.stream import StreamPlan
    from coskad_amd.utils.dataset import AE_TRANS_MATS, PoseFramesRobust
    root, exp = tree
    kw = dict(SR.BASE, seg_len=seg_len, seg_stride=stride, **LAYOUTS[layout])
    ds = _dataset(tree, **dict(seg_len=seg_len, seg_stride=stride, **LAYOUTS[layout]))
    N, V, K = ds.num_samples, ds.V, 5
    items = np.stack([ds[i][0] for i in range(K * N)])
    assert items.dtype == np.float32 and items.shape == (K * N, 2, seg_len, V)
    gathered = PoseFramesRobust(root, split="test", exp_dir=exp, **kw).to_device("cuda").gather(torch.arange(K * N)).cpu().numpy()
    where = _window_of(ds)
    trajs = SR.raw_trajectories(root)
    plan = StreamPlan(4, seg_len, stride)
    flags = (ops.STREAM_KP18 if layout == "kp18" else 0) | (ops.STREAM_HEADLESS if layout == "headless" else 0)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    ring = torch.zeros(4, plan.R, 2, V, device="cuda")
    count = torch.zeros(4, dtype=torch.int32, device="cuda")
    center, scale = (torch.from_numpy(np.asarray(a, dtype=np.float64)).cuda() for a in (ds.scaler.center_, ds.scaler.scale_))
    mats = torch.from_numpy(np.ascontiguousarray(AE_TRANS_MATS)).cuda()
    seen = set()
    for _, tids in SR.clips_of(trajs).items():
        for f, here, rows in SR.frame_events(trajs, tids):
            p = plan.push(f, here)
            m = len(p.ready_slots)
            x = ops.stream_push(torch.from_numpy(rows).cuda(), i32(p.slots).cuda(), i32(p.slots), i32(p.reset).cuda(),
                                i32(p.out_index).cuda(), center, scale, (1080, 720), flags, mats, ring, count, m, seg_len, V, stride)
            assert (x is None) == (m == 0)
            if m == 0:
                continue
            got = x.cpu().numpy().reshape(K, m, 2, seg_len, V)
            for j, (t, first) in enumerate(zip(p.ready_tracks, p.first_frames)):
                s = where[(*t, first)]
                for k in range(K):
                    assert np.array_equal(got[k, j], items[k * N + s]), (t, first, k)
                    assert np.array_equal(_bits(got[k, j]), _bits(gathered[k * N + s])), (t, first, k)
                seen.add(s)
        plan.close()
    assert seen == set(range(N))
    assert count.cpu().tolist() == plan.count                   # the host mirrors the device's row counts


# ---- 4. scores ----------------------------------------------------------------------------------------------------------------

def _lit(cls_name, yaml_name, seed=0, **over):
    """the wrapper at the yaml's default widths with random weights, non-trivial running statistics and a centre, in eval mode"""
    from coskad_amd import lit as L
    from coskad_amd.utils.argparser import init_sub_args
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", yaml_name)), Loader=yaml.FullLoader)
    cfg.update(dict(create_experiment_dir=False, **over))
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(seed)
    lit = getattr(L, cls_name)(args).cuda()
    with torch.no_grad():
        for mod in lit.model.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm) and mod.running_mean is not None:
                mod.running_mean.normal_(0.0, 0.3)
                mod.running_var.uniform_(0.5, 1.5)
        lit.model.c.copy_(0.1 * torch.randn_like(lit.model.c))
        if getattr(lit.model, "inv_cov_matrix", None) is not None:
            a = torch.randn_like(lit.model.inv_cov_matrix)
            lit.model.inv_cov_matrix.copy_(a @ a.T / a.shape[0] + torch.eye(a.shape[0], device=a.device))
    lit.model.eval()
    return lit


WRAPPERS = {"euclidean": ("LitEncoder", "euclidean_encoder.yaml", {}),
            "mahalanobis": ("LitEncoder", "euclidean_encoder.yaml", dict(distance="mahalanobis")),
            "poincare": ("LitEncoder", "hyperbolic_encoder.yaml", {}),
            "autoencoder": ("LitAutoEncoder", "euclidean_autoencoder.yaml", {})}


def _stream_split(tree, lit, ds, K, clip_frames=None):
    """Replays the test split through a StreamScorer.  -> (window scores [K, N] and windows [K N, ...] in the dataset's order, {(k, track,
    frame id): frame score}, {clip: clip vector [K, frames]}), everything on the host."""
    from coskad_amd.stream import StreamScorer
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    where, N = _window_of(ds), ds.num_samples
    sc = StreamScorer(lit, ds.scaler, (1080, 720), max_tracks=4, num_transform=K, clip_frames=clip_frames)
    wins, finals, clips, kept = {}, [], {}, []
    for key, tids in SR.clips_of(trajs).items():
        if clip_frames is not None:
            sc.reset()
        for f, here, rows in SR.frame_events(trajs, tids):
            out = sc.push(f, here, rows.reshape(len(here), 17, 2) if f % 2 else rows)
            kept.append(out)
        kept.append(sc.close())
        if clip_frames is not None:
            clips[key] = sc.clip_scores().cpu().numpy()
    scores = np.zeros((K, N), np.float64)
    x = np.zeros((K * N, 2, ds.T, ds.V), np.float32)
    dtype = None
    frame = {}
    for out in kept:                                            # the only device -> host copies, after the replay
        if out.window_scores is not None:
            dtype = out.window_scores.dtype
            w, xs = out.window_scores.double().cpu().numpy(), out.windows.cpu().numpy()
            for j, (t, first) in enumerate(zip(out.tracks, out.first_frames)):
                scores[:, where[(*t, first)]] = w[:, j]
                for k in range(K):
                    x[k * N + where[(*t, first)]] = xs[k * len(out.tracks) + j]
        if out.frame_scores is not None:
            assert out.frame_scores.dtype == torch.float64
            fs = out.frame_scores.cpu().numpy()
            for q, (t, f) in enumerate(out.final):
                for k in range(K):
                    assert (k, t, f) not in frame
                    frame[(k, t, f)] = fs[k, q]
    return scores, x, frame, clips, dtype


def _batch_scores(lit, x):
    """predict_step's scores of one batch of windows"""
    from coskad_amd.lit import LitAutoEncoder
    n = x.shape[0]
    out = lit.predict_step([torch.from_numpy(x).cuda(), torch.zeros(n, dtype=torch.int64), torch.zeros(n, 4, dtype=torch.int64),
                            torch.zeros(n, x.shape[2], dtype=torch.int32)])
    return out[0] if isinstance(lit, LitAutoEncoder) else lit.window_scores(out[0])


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_streamed_window_scores_are_the_batch_scores(tree, name):
    """12 x 17, default widths: the 30 windows scored one to three at a time by the stream against predict_step on one batch of 30"""
    cls, cfg, over = WRAPPERS[name]
    lit = _lit(cls, cfg, seed=3, **over)
    ds = _dataset(tree)
    assert ds.num_samples == 30
    scores, x, _, _, dtype = _stream_split(tree, lit, ds, 1)
    batch = np.stack([ds[i][0] for i in range(30)])
    assert np.array_equal(_bits(x), _bits(batch.astype(np.float32)))
    want = _batch_scores(lit, batch)
    assert want.dtype == dtype and tuple(want.shape) == (30,)
    want = want.double().cpu().numpy()
    assert np.all(want > 0) and np.array_equal(scores[0], want)


@pytest.mark.parametrize("layout", ["kp18", "headless"])
def test_other_layouts_score_the_batches_the_stream_formed(tree, layout):
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=4, **{"dataset_" + k: v for k, v in LAYOUTS[layout].items()})
    ds = _dataset(tree, **LAYOUTS[layout])
    scores, x, _, _, _ = _stream_split(tree, lit, ds, 2)
    N = ds.num_samples
    assert np.array_equal(x, np.stack([ds[i][0] for i in range(2 * N)]))
    want = _batch_scores(lit, x).double().cpu().numpy().reshape(2, N)
    assert np.array_equal(scores, want)


# ---- 5. frames ----------------------------------------------------------------------------------------------------------------

def test_frame_means_and_clip_vector_are_the_offline_ones(tree):
    from coskad_amd.utils import eval_utils as E
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=5)
    ds, K = _dataset(tree), 3
    N = ds.num_samples
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    fmax = int(max(f.max() for f, _ in trajs.values())) + 3
    assert min(int(f.min()) for f, _ in trajs.values()) >= 1
    scores, _, frame, clips, _ = _stream_split(tree, lit, ds, K, clip_frames=fmax)
    trans = torch.arange(K).repeat_interleave(N)
    meta = torch.from_numpy(ds.segs_meta).repeat(K, 1)
    frames = torch.from_numpy(np.asarray(ds.segs_ids)).repeat(K, 1)
    s = torch.from_numpy(scores.reshape(-1))
    keys, mean = E.person_frame_scores(s, trans, meta, frames, fmax)
    mean = mean.numpy()
    row = {tuple(k): i for i, k in enumerate(keys.tolist())}
    windowed = {tuple(int(v) for v in r[:3]) for r in ds.segs_meta}
    assert len(frame) == K * 63
    for (k, t, f), v in frame.items():
        assert t in windowed                                    # at 12 frames every test track has a window
        assert v == mean[row[(k, *t)], f - 1] and v > 0, (k, t, f)
    lengths = {c: fmax for c in SR.clips_of(trajs)}
    want = E.frame_scores(s, trans, meta, frames, lengths, K, pad_size=-1)
    assert sorted(want) == sorted((k, *c) for k in range(K) for c in lengths)
    for (k, sc, cl), v in want.items():
        assert np.array_equal(clips[(sc, cl)][k], v), (k, sc, cl)


def _row_means(s, n, T, step):
    """float64 restatement: s [n] window scores by END row (entries below R - 1 unused) -> the mean of every row 0 .. n - 1 over the
    windows that cover it, by ascending window start, exact zeros missing, 0 when none is left"""
    R = (T - 1) * step + 1
    out = np.zeros(n, np.float64)
    for i in range(n):
        total, cnt = np.float64(0.0), 0
        for t in range(T - 1, -1, -1):
            e = i + (R - 1) - t * step
            if e < R - 1 or e > n - 1:
                continue
            if s[e] != 0.0:
                total, cnt = total + np.float64(s[e]), cnt + 1
        out[i] = total / np.float64(cnt) if cnt else 0.0
    return out


@pytest.mark.parametrize("T,step,f64", [(8, 1, False), (8, 3, True), (12, 1, True), (24, 1, False)])
def test_frames_launch_against_a_float64_restatement(T, step, f64):
    """two tracks in slots 2 and 0 of three, K = 2, hand-made scores: exact zeros scattered, and every window that covers row 5 of the
    first track is zero.  The second track starts 4 rows later and is shorter; the clip vector is the max of the two."""
    from coskad_amd import ops
    R, K, M = (T - 1) * step + 1, 2, 3
    n = {2: R + 2 * T + 3, 0: R + T}
    start = {2: 0, 0: 4}
    gen = np.random.default_rng(T * 10 + step)
    s = {sl: gen.uniform(0.1, 2.0, (K, n[sl])).astype(np.float32).astype(np.float64 if f64 else np.float32) for sl in n}
    for sl in n:
        s[sl][:, gen.integers(R - 1, n[sl], 5)] = 0.0
    s[2][0, [5 + (R - 1) - t * step for t in range(T)]] = 0.0
    count = torch.zeros(M, dtype=torch.int32, device="cuda")
    wscore = torch.full((M, K, R), float("nan"), dtype=torch.float64, device="cuda")
    frames_total = start[0] + n[0] + n[2]
    clip = torch.zeros(K, frames_total, dtype=torch.float64, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    got = {sl: np.full((K, n[sl]), np.nan) for sl in n}
    for step_i in range(max(start[sl] + n[sl] for sl in n)):
        live = [sl for sl in (2, 0) if start[sl] <= step_i < start[sl] + n[sl]]
        for sl in live:
            count[sl] += 1
        ready = [sl for sl in live if step_i - start[sl] >= R - 1]
        if not ready:
            continue
        e = {sl: step_i - start[sl] for sl in ready}
        sc = torch.from_numpy(np.stack([s[sl][:, e[sl]] for sl in ready], 1).reshape(-1).copy()).cuda()
        fm = ops.stream_frames(sc, i32(ready).cuda(), i32(ready), i32([start[sl] + e[sl] - (R - 1) for sl in ready]).cuda(), count,
                               wscore, clip, T, step)
        assert tuple(fm.shape) == (K, len(ready)) and fm.dtype == torch.float64
        for j, sl in enumerate(ready):
            got[sl][:, e[sl] - (R - 1)] = fm[:, j].cpu().numpy()
    rows = [(sl, i) for sl in (0, 2) for i in range(n[sl] - (R - 1), n[sl])]
    fm = ops.stream_close(i32([sl for sl, _ in rows]).cuda(), i32([sl for sl, _ in rows]), i32([i for _, i in rows]).cuda(),
                          i32([start[sl] + i for sl, i in rows]).cuda(), count, wscore, clip, T, step).cpu().numpy()
    for q, (sl, i) in enumerate(rows):
        got[sl][:, i] = fm[:, q]
    want_clip = np.zeros((K, frames_total))
    for sl in n:
        for k in range(K):
            want = _row_means(s[sl][k].astype(np.float64), n[sl], T, step)
            assert np.array_equal(got[sl][k], want), (sl, k)
            want_clip[k, start[sl]:start[sl] + n[sl]] = np.maximum(want_clip[k, start[sl]:start[sl] + n[sl]], want)
    assert _row_means(s[2][0].astype(np.float64), n[2], T, step)[5] == 0.0 and got[2][0, 5] == 0.0
    assert np.array_equal(clip.cpu().numpy(), want_clip)


def test_track_that_never_filled_a_window_closes_with_zeros(tree):
    from coskad_amd.stream import StreamScorer
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=6)
    root, exp = tree
    ds = _dataset(tree)
    trajs = SR.raw_trajectories(root, "train")
    tid = next(t for t, (f, _) in trajs.items() if len(f) == 9)
    sc = StreamScorer(lit, ds.scaler, (1080, 720), max_tracks=2, num_transform=2, clip_frames=64)
    for f, row in zip(*trajs[tid]):
        out = sc.push(int(f), [tid], row[None])
        assert out.tracks == [] and out.window_scores is None and out.final == []
    out = sc.close()
    assert out.final == [(tid, int(f)) for f in trajs[tid][0]] and tuple(out.frame_scores.shape) == (2, 9)
    assert not out.frame_scores.any() and not sc.clip_scores().any()


# ---- 6. no synchronisation ---------------------------------------------------------------------------------------------------------

def test_push_does_not_synchronise(tree):
    from coskad_amd.stream import StreamScorer
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=7)
    root, _ = tree
    ds = _dataset(tree)
    trajs = SR.raw_trajectories(root)
    tid = next(iter(trajs))
    frames, rows = trajs[tid]
    sc = StreamScorer(lit, ds.scaler, (1080, 720), max_tracks=2, num_transform=5, clip_frames=int(frames.max()) + 1)
    for f, row in zip(frames[:14], rows[:14]):                  # warm: three pushes have scored a window already
        sc.push(int(f), [tid], row[None])
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raised = False
        except RuntimeError:
            raised = True
        if raised:
            for f, row in zip(frames[14:20], rows[14:20]):
                out = sc.push(int(f), [tid], row[None])
                assert out.tracks == [tid] and out.frame_scores is not None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("a host read of a device scalar does not raise under set_sync_debug_mode('error') on this build")
    assert bool((out.window_scores > 0).all())


# ---- 7. the script -----------------------------------------------------------------------------------------------------------------

def _run(cmd):
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    return r.stdout


def _auc(out):
    m = re.search(r"final AUC score: ([0-9.eE+-]+)", out)
    assert m, out[-2000:]
    return float(m.group(1))


def test_stream_cli_prints_the_evaluated_auc(tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), ae_epochs=1)
    path = str(tmp_path / "train.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    _run([sys.executable, "train_COSKAD.py", "--config", path])
    ckpts = sorted(glob.glob(os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"], "*.ckpt")))
    assert ckpts
    path2 = str(tmp_path / "eval.yaml")
    yaml.safe_dump(dict(cfg, load_ckpt=os.path.basename(ckpts[-1])), open(path2, "w"))
    auc_eval = _auc(_run([sys.executable, "eval_COSKAD.py", "--config", path2]))
    out_dir = tmp_path / "streamed"
    auc_stream = _auc(_run([sys.executable, "stream_COSKAD.py", "--config", path2, "--out", str(out_dir)]))
    # the bound tests/test_gpu_score_device.py allows between the host and the device scoring route
    np.testing.assert_allclose(auc_stream, auc_eval, rtol=1e-12)
    files = sorted(p.name for p in out_dir.iterdir())
    assert files == sorted(f"{s}_{c}.npy" for s in (1, 2) for c in (1, 2, 3))
    for p in out_dir.iterdir():
        v = np.load(p)
        assert v.shape == (cfg["dataset_num_transform"], 200) and v.dtype == np.float64 and (v >= 0).all() and v.any()
