"""The camera bank of the online scoring on the GPU (coskad_amd/stream.py `StreamBank`, csrc/stream.hip): two cameras in one
tick give what one `StreamScorer` per camera gives, bit for bit; the resolution is per detection; a camera pushed past its clip vector
leaves its neighbour's alone; the fixed-lag smoothing equals the offline smoothing of the finished vector bit for bit, at kernel level and
through `push`; a tick costs the same number of library calls for 1 and for 4 cameras and never synchronises; stream_COSKAD.py --cameras
prints the line it prints without the flag."""
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
from test_gpu_stream import LAYOUTS, WRAPPERS, _batch_scores, _bits, _dataset, _lit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (1080, 720)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return SR.build_tree(tmp_path_factory.mktemp("morais"), tmp_path_factory.mktemp("exp"))


def _clip_events(tree):
    """[(clip key, [(frame id, [track ids], rows [n, 34])])] of the golden test split, and the largest frame id + 3"""
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    clips = [(key, SR.frame_events(trajs, tids)) for key, tids in SR.clips_of(trajs).items()]
    return clips, int(max(f.max() for f, _ in trajs.values())) + 3


def _host(t):
    return None if t is None else t.cpu().numpy()


def _split(out, cam):
    """the part of a BankOut that belongs to `cam`, as a StreamOut's fields on the host (tracks without the camera)"""
    K = None if out.window_scores is None else out.window_scores.shape[0]
    cols = [j for j, (c, _) in enumerate(out.tracks) if c == cam]
    rows = [q for q, ((c, _), _) in enumerate(out.final) if c == cam]
    m = len(out.tracks)
    return dict(tracks=[out.tracks[j][1] for j in cols], first=[out.first_frames[j] for j in cols],
                scores=None if not cols else _host(out.window_scores)[:, cols],
                windows=None if not cols else _host(out.windows).reshape(K, m, *out.windows.shape[1:])[:, cols],
                final=[(out.final[q][0][1], out.final[q][1]) for q in rows],
                frame=None if not rows else _host(out.frame_scores)[:, rows])


def _whole(out):
    K = None if out.window_scores is None else out.window_scores.shape[0]
    m = len(out.tracks)
    return dict(tracks=list(out.tracks), first=list(out.first_frames), scores=_host(out.window_scores),
                windows=None if not m else _host(out.windows).reshape(K, m, *out.windows.shape[1:]), final=list(out.final),
                frame=_host(out.frame_scores))


def _same(got, want, scores=True):
    assert got["tracks"] == want["tracks"] and got["first"] == want["first"] and got["final"] == want["final"]
    for key in ("windows", "scores", "frame") if scores else ("windows",):
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
            assert np.array_equal(np.ascontiguousarray(got[key]).view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), key


# ---- 1. two cameras in one tick = one scorer per camera --------------------------------------------------------------------------

@pytest.mark.parametrize("name,layout", [("euclidean", "plain"), ("poincare", "plain"), ("autoencoder", "plain"), ("euclidean", "kp18"),
                                         ("euclidean", "headless")])
def test_two_cameras_replay_equals_one_scorer_per_camera(tree, name, layout):
    """the golden test split's two clips as two cameras, tick-interleaved, K = 3, 12 x 17 default widths"""
    from coskad_amd.stream import StreamBank, StreamScorer
    cls, cfg, over = WRAPPERS[name]
    lit = _lit(cls, cfg, seed=11, **dict(over, **{"dataset_" + k: v for k, v in LAYOUTS[layout].items()}))
    ds = _dataset(tree, **LAYOUTS[layout])
    clips, fmax = _clip_events(tree)
    assert len(clips) == 2
    K = 3
    bank = StreamBank(lit, ds.scaler, {c: dict(vid_res=RES, clip_frames=fmax) for c in range(2)}, max_tracks=4, num_transform=K)
    alone = [StreamScorer(lit, ds.scaler, RES, max_tracks=4, num_transform=K, clip_frames=fmax) for _ in range(2)]
    got, want, formed = [], [], []
    for tick in range(max(len(ev) for _, ev in clips)):
        batch = {c: clips[c][1][tick] for c in range(2) if tick < len(clips[c][1])}
        out = bank.push(batch)
        formed.append(out)
        for c in batch:
            got.append(_split(out, c))
            want.append(_whole(alone[c].push(*batch[c])))
    assert any(len(set(c for c, _ in o.tracks)) == 2 for o in formed)          # some launches carried windows of both cameras
    for c in range(2):
        got.append(_split(bank.finish(c), c))
        want.append(_whole(alone[c].close()))
    plain = layout == "plain"
    assert sum(len(w["tracks"]) for w in want) == ds.num_samples and sum(len(w["final"]) for w in want) == 63
    for g, w in zip(got, want):
        _same(g, w, scores=plain)
    if plain:
        for c in range(2):
            a, b = bank.clip_scores(c).cpu().numpy(), alone[c].clip_scores().cpu().numpy()
            assert a.any() and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    else:       # the bar of test_other_layouts_score_the_batches_the_stream_formed: predict_step on the batch the bank formed
        for o in formed:
            if o.windows is not None:
                ref = _batch_scores(lit, o.windows.cpu().numpy()).double().cpu().numpy().reshape(K, -1)
                assert np.array_equal(o.window_scores.double().cpu().numpy(), ref)


# ---- 2. the resolution is per detection -------------------------------------------------------------------------------------------

def test_resolution_is_per_detection(tree):
    """cameras at (1080, 720) and (640, 360) see the same raw rows in the same launch; each one's windows are those of a StreamScorer
    of its resolution"""
    from coskad_amd.stream import StreamBank, StreamScorer
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=12)
    ds = _dataset(tree)
    clips, _ = _clip_events(tree)
    res = {"A": (1080, 720), "B": (640, 360)}
    bank = StreamBank(lit, ds.scaler, {c: dict(vid_res=res[c]) for c in res}, max_tracks=8, num_transform=2)
    alone = {c: StreamScorer(lit, ds.scaler, res[c], max_tracks=4, num_transform=2) for c in res}
    got, want = {c: [] for c in res}, {c: [] for c in res}
    for _, events in clips:
        for ev in events:
            out = bank.push({c: ev for c in res})
            assert len(out.tracks) == 2 * len([1 for c, _ in out.tracks if c == "A"])
            for c in res:
                got[c].append(_split(out, c))
                want[c].append(_whole(alone[c].push(*ev)))
        for c in res:
            got[c].append(_split(bank.finish(c), c))
            want[c].append(_whole(alone[c].close()))
            bank.reset(c)
    for c in res:
        for g, w in zip(got[c], want[c]):
            _same(g, w)
    a = np.concatenate([g["windows"] for g in got["A"] if g["windows"] is not None], 1)
    b = np.concatenate([g["windows"] for g in got["B"] if g["windows"] is not None], 1)
    assert a.shape == b.shape and a.shape[1] == 30
    assert all(not np.array_equal(a[:, j], b[:, j]) for j in range(30))       # a kernel that ignored `res` would make them equal


# ---- 3. clip segments stay apart --------------------------------------------------------------------------------------------------

def test_a_camera_pushed_past_its_clip_frames_leaves_its_neighbour_alone(tree):
    from coskad_amd.stream import StreamBank
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=13)
    ds = _dataset(tree)
    clips, fmax = _clip_events(tree)
    events = max((ev for _, ev in clips), key=len)
    short = events[0][0] + 14                                    # camera a's vector ends in the middle of the frames that score
    assert events[-1][0] > short + 5

    def run(cams):
        bank = StreamBank(lit, ds.scaler, {"a": dict(vid_res=RES, clip_frames=short), "b": dict(vid_res=RES, clip_frames=fmax)},
                          max_tracks=8, num_transform=2)
        for ev in events:
            bank.push({c: ev for c in cams})
        for c in cams:
            bank.finish(c)
        return bank

    both, only_b = run(["a", "b"]), run(["b"])
    b = both.clip_scores("b").cpu().numpy()
    assert (b[:, short:] > 0).any() and (b[:, :short] > 0).any()
    assert np.array_equal(b.view(np.uint8), only_b.clip_scores("b").cpu().numpy().view(np.uint8))
    a = both.clip_scores("a").cpu().numpy()
    assert a.shape == (2, short) and np.array_equal(a, b[:, :short])           # and camera a kept its own frames
    assert both.bank.clip_index("a", short) == short - 1 and both.bank.clip_index("a", short + 1) == -1


# ---- 4. smoothing, kernel level ------------------------------------------------------------------------------------------------------

SEGS = (37, 121, 400)


@pytest.fixture(scope="module")
def smooth_case():
    """K = 2, three segments in one flat buffer: non-negative values with exact zeros (runs of them, and isolated ones); the offline
    smoothing of the finished vector, computed once"""
    from coskad_amd import ops
    from coskad_amd.utils.score_plan import gaussian_taps, segment_tiles
    gen = np.random.default_rng(5)
    F = sum(SEGS)
    raw = gen.uniform(0.05, 3.0, (2, F))
    raw[gen.random((2, F)) < 0.1] = 0.0
    raw[0, 40:75] = 0.0
    raw[:, 160:175] = 0.0
    raw[1, 540:] = 0.0
    bounds = np.concatenate([[0], np.cumsum(SEGS)])
    segments = [(int(bounds[i]), int(bounds[i + 1])) for i in range(len(SEGS))]
    taps = torch.from_numpy(gaussian_taps()).cuda()
    tiles = torch.from_numpy(segment_tiles(segments).astype(np.int32)).cuda()
    per_t, mean = ops.score_smooth(torch.from_numpy(raw).cuda(), tiles, taps)
    return raw, segments, taps, per_t.cpu().numpy(), mean.cpu().numpy()


def test_fixed_lag_smoothing_equals_the_offline_smoothing(smooth_case):
    """emitted at watermarks 1, 120, 121, 122, 250, 399 -- with everything at and beyond the watermark still unknown (NaN) -- then the
    tail at finish: the pieces concatenated are coskad_score_smooth_f64's values of the finished vector, bit for bit"""
    from coskad_amd import ops
    from coskad_amd.stream import emittable
    from coskad_amd.utils.eval_utils import score_process
    raw, segments, taps, want_t, want_mean = smooth_case
    K, F = raw.shape
    done = [0] * len(segments)
    pieces_t, pieces_m = [[] for _ in segments], [[] for _ in segments]
    counts = []

    def emit(known, upto):
        rows = [(a, b - a, i) for s, (a, b) in enumerate(segments) for i in range(done[s], upto[s])]
        counts.append([upto[s] - done[s] for s in range(len(segments))])
        if not rows:
            return
        items = torch.tensor(rows, dtype=torch.int32)
        per_t, mean = ops.stream_smooth(torch.from_numpy(known).cuda(), items.cuda(), items.reshape(-1), taps)
        per_t, mean = per_t.cpu().numpy(), mean.cpu().numpy()
        assert per_t.shape == (K, len(rows)) and mean.shape == (len(rows),)
        at = 0
        for s in range(len(segments)):
            n = upto[s] - done[s]
            pieces_t[s].append(per_t[:, at:at + n])
            pieces_m[s].append(mean[at:at + n])
            at, done[s] = at + n, upto[s]

    for W in (1, 120, 121, 122, 250, 399):
        known = raw.copy()
        for a, b in segments:
            known[:, a + min(W, b - a):b] = np.nan
        emit(known, [emittable(min(W, b - a)) for a, b in segments])
    assert counts == [[0, 0, 0], [0, 0, 0], [0, 1, 1], [0, 0, 1], [0, 0, 128], [0, 0, 149]]
    emit(raw, [b - a for a, b in segments])
    assert counts[-1] == [37, 120, 121]                         # the 37-frame segment comes out whole at finish
    for s, (a, b) in enumerate(segments):
        got_t, got_m = np.concatenate(pieces_t[s], 1), np.concatenate(pieces_m[s])
        assert not np.isnan(got_t).any()
        assert np.array_equal(got_t.view(np.uint64), want_t[:, a:b].view(np.uint64)), s
        assert np.array_equal(got_m.view(np.uint64), want_mean[a:b].view(np.uint64)), s
        assert np.array_equal(got_m.view(np.uint64), np.mean(got_t, 0).view(np.uint64)), s
        for k in range(K):      # the bound tests/test_gpu_score_device.py holds the device smoothing to
            np.testing.assert_allclose(got_t[k], score_process(raw[k, a:b]), rtol=1e-12, atol=0)


# ---- 5. smoothing through push -------------------------------------------------------------------------------------------------------

def test_smoothed_scores_through_push(tree):
    """one camera, 300 frames of golden rows on two tracks: one is closed by the caller at frame 150 and comes back as a new track, the
    other stops at frame 220 and is closed by idle_close = 5"""
    from coskad_amd import ops
    from coskad_amd.stream import StreamBank
    from coskad_amd.utils.score_plan import gaussian_taps, segment_tiles
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=14)
    ds = _dataset(tree)
    root, _ = tree
    rows = [r for _, r in SR.raw_trajectories(root).values()]
    K, n = 2, 300
    bank = StreamBank(lit, ds.scaler, {"cam": dict(vid_res=RES, clip_frames=n)}, max_tracks=3, num_transform=K, smooth=True, idle_close=5)
    outs, idle_final = [], []
    for f in range(1, n + 1):
        here = ([1] if f <= 150 or f > 170 else []) + ([2] if f <= 220 else [])
        out = bank.push({"cam": (f, here, np.stack([rows[t - 1][f % len(rows[t - 1])] for t in here]) if here else np.zeros((0, 34)))})
        outs.append(out)
        if f == 150:
            outs.append(bank.close("cam", [1]))
        if f == 226:
            idle_final = [x for x in out.final if x[0] == ("cam", 2)]
    assert [fr for _, fr in idle_final] == list(range(210, 221)) and bank.plan.live == [("cam", 1)]
    early = sum(c for o in outs for _, _, c in o.smoothed)
    assert early == bank.watermark("cam") - 120 and early > 150
    outs.append(bank.finish("cam"))
    at, per_t, mean = 0, [], []
    for o in outs:
        for cam, first, count in o.smoothed:
            assert cam == "cam" and first == at and count > 0
            at += count
        if o.smoothed:
            assert o.smoothed_scores.dtype == torch.float64 and tuple(o.smoothed_scores.shape) == (K, sum(c for _, _, c in o.smoothed))
            per_t.append(o.smoothed_scores)
            mean.append(o.smoothed_mean)
    assert at == n
    clip = bank.clip_scores("cam")
    assert bool((clip > 0).any(1).all())
    tiles = torch.from_numpy(segment_tiles([(0, n)]).astype(np.int32)).cuda()
    want_t, want_mean = ops.score_smooth(clip, tiles, torch.from_numpy(gaussian_taps()).cuda())
    assert torch.equal(torch.cat(per_t, 1).view(torch.int64), want_t.view(torch.int64))
    assert torch.equal(torch.cat(mean).view(torch.int64), want_mean.view(torch.int64))


# ---- 6. calls per tick, no synchronisation -------------------------------------------------------------------------------------------

def test_a_tick_costs_the_same_calls_for_one_and_four_cameras_and_never_synchronises(tree):
    from coskad_amd import _lib, ops
    from coskad_amd.stream import StreamBank
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=15)
    ds = _dataset(tree)
    root, _ = tree
    rows = next(iter(SR.raw_trajectories(root).values()))[1]
    banks = {C: StreamBank(lit, ds.scaler, {c: dict(vid_res=RES, clip_frames=200) for c in range(C)}, max_tracks=2 * C, num_transform=3,
                           smooth=True) for C in (1, 4)}

    def tick(C, f):
        kp = np.stack([rows[f % len(rows)], rows[(f + 5) % len(rows)]])
        return banks[C].push({c: (f, [0, 1], kp) for c in range(C)})

    for f in range(1, 136):                                      # warm: from frame 132 on the watermark (f - 11) passes 120 every tick
        for C in banks:
            out = tick(C, f)
    assert len(out.tracks) == 8 and [c for _, _, c in out.smoothed] == [1, 1, 1, 1]
    calls, real = [0], _lib.call

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    per_tick = {}
    _lib.call = ops.call = counting                             # as tools/bench_stream.py counts `calls`
    try:
        for C in banks:
            calls[0] = 0
            out = tick(C, 136)
            per_tick[C] = calls[0]
            assert out.smoothed_scores is not None and out.frame_scores is not None
    finally:
        _lib.call = ops.call = real
    assert per_tick[1] == per_tick[4] and per_tick[1] >= 3, per_tick
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
            for f in range(137, 143):
                out = tick(4, f)
                assert len(out.tracks) == 8 and len(out.final) == 8 and len(out.smoothed) == 4
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("a host read of a device scalar does not raise under set_sync_debug_mode('error') on this build")
    assert bool((out.window_scores > 0).all()) and bool(torch.isfinite(out.smoothed_scores).all())


# ---- 7. the script -----------------------------------------------------------------------------------------------------------------

def _run(cmd):
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    return r.stdout


def test_stream_cli_with_cameras_prints_the_same_line(tmp_path):
    from coskad_amd import lit as L
    from coskad_amd.utils.argparser import init_sub_args
    from coskad_amd.utils.eval_utils import score_process
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), create_experiment_dir=False, load_ckpt="random.ckpt")
    args, *_ = init_sub_args(Namespace(**cfg))
    torch.manual_seed(21)
    lit = L.LitEncoder(args)                                    # no training run: a randomly initialised wrapper
    with torch.no_grad():
        lit.model.c.copy_(0.1 * torch.randn_like(lit.model.c))
    os.makedirs(os.path.join(args.exp_dir, args.dataset_choice, args.dir_name), exist_ok=True)
    L.save_checkpoint(lit, os.path.join(args.exp_dir, args.dataset_choice, args.dir_name, "random.ckpt"))
    path = str(tmp_path / "eval.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    line = re.compile(r"^final AUC score: .*$", re.M)
    plain = line.search(_run([sys.executable, "stream_COSKAD.py", "--config", path, "--out", str(tmp_path / "plain")]))
    out = _run([sys.executable, "stream_COSKAD.py", "--config", path, "--cameras", "3", "--out", str(tmp_path / "raw"), "--smoothed-out",
                str(tmp_path / "smoothed")])
    assert plain and line.search(out) and line.search(out).group(0) == plain.group(0)
    names = sorted(f"{s}_{c}" for s in (1, 2) for c in (1, 2, 3))
    assert sorted(p.name for p in (tmp_path / "raw").iterdir()) == [f"{k}.npy" for k in names]
    assert sorted(p.name for p in (tmp_path / "smoothed").iterdir()) == [f"{k}_smoothed.npy" for k in names]
    for k in names:
        raw, sm = np.load(tmp_path / "raw" / f"{k}.npy"), np.load(tmp_path / "smoothed" / f"{k}_smoothed.npy")
        assert np.array_equal(raw, np.load(tmp_path / "plain" / f"{k}.npy")) and raw.any()
        assert sm.shape == raw.shape and sm.dtype == np.float64
        for t in range(raw.shape[0]):
            np.testing.assert_allclose(sm[t], score_process(raw[t]), rtol=1e-12, atol=0)
