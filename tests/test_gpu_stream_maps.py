"""Per-joint maps of the stream on the GPU (coskad_amd/stream.py `maps=True`, csrc/stream.hip): the maps launches against a
float64 numpy restatement on random window maps (ring wrap, slot reuse, a track without a window, a dirty state); the golden test split
replayed frame by frame gives the offline route's person-frame maps bit for bit, for the one-class encoders and the autoencoder, while
every score stays the one of the stream without maps; a bank tick equals one scorer per camera; a push with maps never synchronises;
stream_COSKAD.py writes eval_COSKAD.py's map files byte for byte."""
import glob
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import stream_refs as SR
from test_gpu_stream import WRAPPERS, _auc, _dataset, _lit, _run, _stream_split, _window_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (1080, 720)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return SR.build_tree(tmp_path_factory.mktemp("morais"), tmp_path_factory.mktemp("exp"))


def _same_bits(a, b):
    """`==` on the bit patterns, NaN positions equal"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


# ---- 1. the launches against a float64 restatement --------------------------------------------------------------------------------

def _row_maps(w, n, T, step, V):
    """float64 restatement: w {end row e: map [T, V] float32} of one (track, transformation) -> [n, V]: the mean of every row over the
    windows that cover it -- window e holds row e - (T - 1 - t) step at position t -- summed in ascending window start, an exact 0
    counted like any value, NaN where no window covers the row"""
    out = np.full((n, V), np.nan, np.float64)
    for i in range(n):
        total, cnt = np.zeros(V, np.float64), 0
        for e in sorted(w):
            for t in range(T):
                if e - (T - 1 - t) * step == i:
                    total = total + w[e][t].astype(np.float64)
                    cnt += 1
        if cnt:
            out[i] = total / np.float64(cnt)
    return out


def _tracks(T, step):
    """(name, slot, first tick, rows): a and b wrap their rings (R + T + 3 rows) from different ticks; c is closed in mid-run after two
    windows, with a ring full of sums (at step > 1 no window covers some of its trailing rows), and d takes its slot in the tick that
    closes c; e closes before it ever filled a window and f follows it"""
    R = (T - 1) * step + 1
    n = R + T + 3
    return [("a", 0, 0, n), ("b", 3, 2, n), ("c", 5, 1, R + 1), ("d", 5, 1 + R + 1, n), ("e", 1, 3, R - 2), ("f", 1, 3 + R - 2, n)]


def _run_maps(T, step, V, dirty):
    """The scenario of `_tracks` through ops.stream_maps / ops.stream_maps_close, M = 6 slots, K = 2.  -> ({track: window maps
    {k: {e: [T, V]}}}, {track: frame maps [K, rows, V]}), everything on the host; one device -> host copy per launch, after the run."""
    from coskad_amd import ops
    M, K = 6, 2
    R = (T - 1) * step + 1
    tracks = _tracks(T, step)
    gen = np.random.default_rng(1000 * T + 10 * step + V)
    wm = {}
    for name, _, _, n in tracks:
        wm[name] = {k: {e: gen.standard_normal((T, V)).astype(np.float32) for e in range(R - 1, n)} for k in range(K)}
        for k in range(K):
            for e in list(wm[name][k])[::3]:                    # exact zeros count: scattered, and a whole window of them
                wm[name][k][e][gen.integers(0, T, 4), gen.integers(0, V, 4)] = 0.0
    wm["a"][0][R + 1][:] = 0.0
    wm["b"][1][R - 1][:] = -0.0
    state = ops.stream_maps_state(M, K, T, V, step, "cuda")
    assert state.dtype == torch.float64 and state.numel() * 8 == ops.stream_maps_state_bytes(M, K, T, V, step)
    if dirty:                                                    # what a previous tenant may have left: the state is keyed on `count`
        state.copy_(torch.from_numpy(gen.standard_normal(state.numel()) * 1e6))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    count = [0] * M
    kept = []
    for tick in range(max(s + n for _, _, s, n in tracks) + 1):
        closing = [tr for tr in tracks if tr[2] + tr[3] == tick]
        if closing:                                              # before the slot's next push, as the stream closes
            rows = [(tr, i) for tr in closing for i in range(tr[3] - min(tr[3], R - 1), tr[3])]
            sl = [tr[1] for tr, _ in rows]
            fm = ops.stream_maps_close(i32(sl).cuda(), i32(sl), i32([i for _, i in rows]).cuda(), i32(count).cuda(), state, K, T, V, step)
            assert tuple(fm.shape) == (K, len(rows), V) and fm.dtype == torch.float64
            kept.append(([(tr[0], i) for tr, i in rows], fm))
        live = [tr for tr in tracks if tr[2] <= tick < tr[2] + tr[3]]
        for name, sl, s, n in live:
            count[sl] = 1 if tick == s else count[sl] + 1        # the push launch: a track's first row resets its count
        ready = [tr for tr in live if tick - tr[2] >= R - 1]
        if not ready:
            continue
        m = len(ready)
        maps = np.stack([wm[tr[0]][k][tick - tr[2]] for k in range(K) for tr in ready])
        sl = [tr[1] for tr in ready]
        fm = ops.stream_maps(torch.from_numpy(maps).cuda(), i32(sl).cuda(), i32(sl), i32(count).cuda(), state, K, T, V, step)
        assert tuple(fm.shape) == (K, m, V) and fm.dtype == torch.float64
        kept.append(([(tr[0], tick - tr[2] - (R - 1)) for tr in ready], fm))
    got = {name: np.full((K, n, V), -7.0) for name, _, _, n in tracks}
    for keys, fm in kept:
        fm = fm.cpu().numpy()
        for q, (name, i) in enumerate(keys):
            assert (got[name][:, i] == -7.0).all()               # every row becomes final once
            got[name][:, i] = fm[:, q]
    return wm, got


@pytest.mark.parametrize("V", [14, 17])
@pytest.mark.parametrize("T,step", [(8, 1), (8, 3), (12, 1), (24, 1)])
def test_maps_launches_against_a_float64_restatement(T, step, V):
    wm, got = _run_maps(T, step, V, dirty=False)
    R = (T - 1) * step + 1
    for name, _, _, n in _tracks(T, step):
        for k in (0, 1):
            want = _row_maps(wm[name][k], n, T, step, V)
            assert _same_bits(got[name][k], want), (name, k)
        if n >= R:
            assert not np.isnan(got[name][:, :n - (R - 1)]).any()        # a row made final by a window is covered by that window
    assert np.isnan(got["e"]).all() and got["e"].shape[1] == R - 2          # never filled a window
    # c's two windows end at rows R - 1 and R: at step 3 they miss every third of the rows below R - 1
    assert np.isnan(got["c"]).any() == (step > 1) and not np.isnan(got["c"][:, R - 1:]).any()
    # d and f took the slots of c and e, rings full of their sums: the equality above with restatements of d's and f's OWN windows is
    # the check that none of those sums is left
    # the whole-zero window counts: the rows it covers differ from the mean without it
    i = R + 1 - (T - 1) * step
    others = {e: v for e, v in wm["a"][0].items() if e != R + 1}
    assert not _same_bits(got["a"][0, i], _row_maps(others, i + 1, T, step, V)[i])
    # two runs agree bit for bit, and a state full of a former tenant's numbers changes nothing
    _, again = _run_maps(T, step, V, dirty=False)
    _, dirty = _run_maps(T, step, V, dirty=True)
    for name in got:
        assert _same_bits(again[name], got[name]) and _same_bits(dirty[name], got[name]), name


# ---- 2. replay = offline --------------------------------------------------------------------------------------------------------------

def _replay_maps(tree, lit, ds, K, clip_frames, stride=1):
    """The test split through StreamScorer(maps=True).  -> (window scores [K, N], window maps [K N, T, V] in the dataset's order,
    {(k, track, frame id): frame score}, {(k, track, frame id): frame map [V]}, {clip: clip vector}), on the host after the replay."""
    from coskad_amd.stream import StreamScorer
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    where, N = _window_of(ds), ds.num_samples
    sc = StreamScorer(lit, ds.scaler, RES, max_tracks=4, seg_stride=stride, num_transform=K, clip_frames=clip_frames, maps=True)
    kept, clips = [], {}
    for key, tids in SR.clips_of(trajs).items():
        sc.reset()
        for f, here, rows in SR.frame_events(trajs, tids):
            kept.append(sc.push(f, here, rows))
        kept.append(sc.close())
        clips[key] = sc.clip_scores().cpu().numpy()
    scores = np.zeros((K, N), np.float64)
    wmaps = np.zeros((K * N, ds.T, ds.V), np.float32)
    frame, fmap = {}, {}
    for out in kept:
        m = len(out.tracks)
        assert (out.window_maps is None) == (m == 0) and (out.frame_maps is None) == (not out.final)
        if m:
            assert tuple(out.window_maps.shape) == (K * m, ds.T, ds.V) and out.window_maps.dtype == torch.float32
            w, wmap = out.window_scores.double().cpu().numpy(), out.window_maps.cpu().numpy()
            for j, (t, first) in enumerate(zip(out.tracks, out.first_frames)):
                scores[:, where[(*t, first)]] = w[:, j]
                for k in range(K):
                    wmaps[k * N + where[(*t, first)]] = wmap[k * m + j]
        if out.final:
            assert tuple(out.frame_maps.shape) == (K, len(out.final), ds.V) and out.frame_maps.dtype == torch.float64
            fs, fm = out.frame_scores.cpu().numpy(), out.frame_maps.cpu().numpy()
            for q, (t, f) in enumerate(out.final):
                for k in range(K):
                    assert (k, t, f) not in fmap
                    frame[(k, t, f)], fmap[(k, t, f)] = fs[k, q], fm[k, q]
    return scores, wmaps, frame, fmap, clips


def _check_replay(tree, lit, ds, K, stride, window_map):
    """the streamed maps against `window_map` on ONE batch of all windows + eval_utils.attribution_frames_device on the scoring plan's
    window table; the scores against the stream without maps"""
    from coskad_amd.utils import eval_utils as E
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    N = ds.num_samples
    fmax = int(max(f.max() for f, _ in trajs.values())) + 3
    scores, wmaps, frame, fmap, clips = _replay_maps(tree, lit, ds, K, fmax, stride)
    batch = torch.from_numpy(np.stack([ds[i][0] for i in range(K * N)])).cuda()
    attr = window_map(batch)
    assert tuple(attr.shape) == (K * N, ds.T, ds.V) and attr.dtype == torch.float32
    assert _same_bits(wmaps, attr.cpu().numpy()) and np.abs(wmaps).max() > 0
    trans = torch.arange(K).repeat_interleave(N)
    meta = torch.from_numpy(ds.segs_meta).repeat(K, 1)
    frames = torch.from_numpy(np.asarray(ds.segs_ids)).repeat(K, 1)
    plan = E.ScorePlan(trans, meta, frames, {c: np.zeros(fmax) for c in SR.clips_of(trajs)}, K, device="cuda")
    want = E.attribution_frames_device(attr, frames, plan).cpu().numpy()
    rp = plan.row_ptr.cpu().numpy()
    row = {tuple(int(v) for v in key): int(rp[p]) for p, key in enumerate(plan.person_keys)}
    windowed = {tuple(int(v) for v in r[:3]) for r in ds.segs_meta}
    assert len(fmap) == K * 63
    covered = 0
    for (k, t, f), v in fmap.items():
        if t not in windowed:                                   # a track without a window is no person of the offline plan
            assert np.isnan(v).all()
            continue
        assert _same_bits(v, want[row[(k, *t)] + f - 1]), (k, t, f)
        covered += int(not np.isnan(v).any())
    assert covered == int((~np.isnan(want).any(1)).sum()) > 0   # every person-frame the offline route has a map for was streamed
    # window scores, frame scores and the clip vector: the stream's without maps, bit for bit
    scores0, _, frame0, clips0, _ = _stream_split(tree, lit, ds, K, clip_frames=fmax) if stride == 1 else \
        _plain_split(tree, lit, ds, K, fmax, stride)
    assert _same_bits(scores, scores0) and scores.any()
    assert frame.keys() == frame0.keys() and all(_same_bits(np.float64(frame[key]), np.float64(frame0[key])) for key in frame)
    assert clips.keys() == clips0.keys() and all(_same_bits(clips[c], clips0[c]) for c in clips)


def _plain_split(tree, lit, ds, K, fmax, stride):
    """`_stream_split` at a seg_stride other than 1: the same replay through StreamScorer(maps=False)"""
    from coskad_amd.stream import StreamScorer
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    where, N = _window_of(ds), ds.num_samples
    sc = StreamScorer(lit, ds.scaler, RES, max_tracks=4, seg_stride=stride, num_transform=K, clip_frames=fmax)
    kept, clips = [], {}
    for key, tids in SR.clips_of(trajs).items():
        sc.reset()
        for f, here, rows in SR.frame_events(trajs, tids):
            kept.append(sc.push(f, here, rows))
        kept.append(sc.close())
        clips[key] = sc.clip_scores().cpu().numpy()
    scores, frame = np.zeros((K, N), np.float64), {}
    for out in kept:
        assert out.frame_maps is None and out.window_maps is None
        if out.tracks:
            w = out.window_scores.double().cpu().numpy()
            for j, (t, first) in enumerate(zip(out.tracks, out.first_frames)):
                scores[:, where[(*t, first)]] = w[:, j]
        if out.final:
            fs = out.frame_scores.cpu().numpy()
            for q, (t, f) in enumerate(out.final):
                for k in range(K):
                    frame[(k, t, f)] = fs[k, q]
    return scores, None, frame, clips, None


@pytest.mark.parametrize("name", ["euclidean", "poincare"])
def test_encoder_replay_equals_the_offline_attribution(tree, name):
    """12 x 17, `linear` projector, K = 2: lit.window_attribution on one batch of all windows + attribution_frames_device"""
    cls, cfg, over = WRAPPERS[name]
    lit = _lit(cls, cfg, seed=21, **over)
    assert lit.model.projector == "linear"
    ds = _dataset(tree)
    assert (ds.T, ds.V, ds.num_samples) == (12, 17, 30)
    _check_replay(tree, lit, ds, 2, 1, lambda x: lit.window_attribution(x)[2])


def test_autoencoder_replay_equals_the_offline_error_map(tree):
    """8 frames at seg_stride 3 (a ring of 22 rows), 'rec+hyp': lit.window_error_map on one batch + attribution_frames_device"""
    cls, cfg, over = WRAPPERS["autoencoder"]
    lit = _lit(cls, cfg, seed=22, dataset_seg_len=8, **over)
    lit.score_type = 'rec+hyp'
    ds = _dataset(tree, seg_len=8, seg_stride=3)
    assert (ds.T, ds.V) == (8, 17) and ds.num_samples > 0
    _check_replay(tree, lit, ds, 2, 3, lambda x: lit.window_error_map(x)[1])


# ---- 3. a bank tick = one scorer per camera -----------------------------------------------------------------------------------------

def _host(t):
    return None if t is None else t.cpu().numpy()


def test_bank_with_maps_equals_one_scorer_per_camera(tree):
    """the golden test split's two clips as two cameras in one tick, K = 2, `finish` included: every field of the bank's output is the
    scorers', the maps among them, and a tick with windows of both cameras still issued ONE maps launch"""
    from coskad_amd import _lib, ops
    from coskad_amd.stream import StreamBank, StreamScorer
    lit = _lit(*WRAPPERS["euclidean"][:2], seed=23)
    ds = _dataset(tree)
    root, _ = tree
    trajs = SR.raw_trajectories(root)
    clips = [SR.frame_events(trajs, tids) for _, tids in SR.clips_of(trajs).items()]
    fmax = int(max(f.max() for f, _ in trajs.values())) + 3
    assert len(clips) == 2
    K, V = 2, ds.V
    bank = StreamBank(lit, ds.scaler, {c: dict(vid_res=RES, clip_frames=fmax) for c in range(2)}, max_tracks=4, num_transform=K, maps=True)
    alone = [StreamScorer(lit, ds.scaler, RES, max_tracks=4, num_transform=K, clip_frames=fmax, maps=True) for _ in range(2)]
    calls = []
    real = _lib.call

    def counting(name, *a, **kw):
        calls.append(name)
        return real(name, *a, **kw)
    pairs, launches = [], []
    for tick in range(max(len(ev) for ev in clips)):
        batch = {c: clips[c][tick] for c in range(2) if tick < len(clips[c])}
        calls.clear()
        ops.call = counting
        try:
            out = bank.push(batch)
        finally:
            ops.call = real
        launches.append((len({c for c, _ in out.tracks}), calls.count("coskad_stream_maps_f64")))
        pairs += [(out, c, alone[c].push(*batch[c])) for c in batch]
    pairs += [(bank.finish(c), c, alone[c].close()) for c in range(2)]
    assert (2, 1) in launches and all(n == (1 if cams else 0) for cams, n in launches)
    finals = 0
    for out, cam, want in pairs:
        cols = [j for j, (c, _) in enumerate(out.tracks) if c == cam]
        rows = [q for q, ((c, _), _) in enumerate(out.final) if c == cam]
        assert [out.tracks[j][1] for j in cols] == want.tracks and [(out.final[q][0][1], out.final[q][1]) for q in rows] == want.final
        m = len(out.tracks)
        if cols:
            assert _same_bits(_host(out.window_scores)[:, cols], _host(want.window_scores))
            assert _same_bits(_host(out.window_maps).reshape(K, m, ds.T, V)[:, cols], _host(want.window_maps).reshape(K, len(cols), ds.T, V))
        else:
            assert want.window_maps is None
        if rows:
            assert tuple(out.frame_maps.shape) == (K, len(out.final), V)
            assert _same_bits(_host(out.frame_scores)[:, rows], _host(want.frame_scores))
            assert _same_bits(_host(out.frame_maps)[:, rows], _host(want.frame_maps))
            finals += len(rows)
        else:
            assert want.frame_maps is None
    assert finals == 63
    for c in range(2):
        assert _same_bits(_host(bank.clip_scores(c)), _host(alone[c].clip_scores()))


# ---- 4. no synchronisation -------------------------------------------------------------------------------------------------------------

def test_push_with_maps_does_not_synchronise(tree):
    from coskad_amd.stream import StreamScorer
    lit = _lit("LitEncoder", "euclidean_encoder.yaml", seed=7)
    root, _ = tree
    ds = _dataset(tree)
    trajs = SR.raw_trajectories(root)
    tid = next(iter(trajs))
    frames, rows = trajs[tid]
    sc = StreamScorer(lit, ds.scaler, (1080, 720), max_tracks=2, num_transform=5, clip_frames=int(frames.max()) + 1, maps=True)
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
                assert out.tracks == [tid] and out.frame_scores is not None and out.frame_maps is not None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("a host read of a device scalar does not raise under set_sync_debug_mode('error') on this build")
    assert bool((out.window_scores > 0).all()) and not bool(torch.isnan(out.frame_maps).any())


# ---- 5. the script -----------------------------------------------------------------------------------------------------------------------

def test_stream_cli_writes_the_evaluated_attribution_maps(tmp_path):
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(exp_dir=str(tmp_path / "ckpt"), ae_epochs=1)
    path = str(tmp_path / "train.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    _run([sys.executable, "train_COSKAD.py", "--config", path])
    ckpts = sorted(glob.glob(os.path.join(cfg["exp_dir"], cfg["dataset_choice"], cfg["dir_name"], "*.ckpt")))
    assert ckpts
    path2 = str(tmp_path / "eval.yaml")
    yaml.safe_dump(dict(cfg, load_ckpt=os.path.basename(ckpts[-1])), open(path2, "w"))
    a, b, c = (tmp_path / d for d in "ABC")
    auc_eval = _auc(_run([sys.executable, "eval_COSKAD.py", "--config", path2, "--attribution-dir", str(a)]))
    auc_plain = _auc(_run([sys.executable, "stream_COSKAD.py", "--config", path2]))
    auc_stream = _auc(_run([sys.executable, "stream_COSKAD.py", "--config", path2, "--attribution-dir", str(b)]))
    auc_bank = _auc(_run([sys.executable, "stream_COSKAD.py", "--config", path2, "--cameras", "2", "--attribution-dir", str(c)]))
    assert auc_stream == auc_plain == auc_bank                  # the printed line does not change with the maps
    np.testing.assert_allclose(auc_stream, auc_eval, rtol=1e-12)        # the bound of test_stream_cli_prints_the_evaluated_auc
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(f"{s}_{cl}_{kind}.npy" for s in (1, 2) for cl in (1, 2, 3) for kind in ("attribution", "persons"))
    for other in (b, c):
        assert sorted(p.name for p in other.iterdir()) == names
        for n in names:
            assert (a / n).read_bytes() == (other / n).read_bytes(), (other.name, n)
    v = np.load(a / "1_1_attribution.npy")
    assert v.dtype == np.float32 and v.ndim == 3 and v.shape[1:] == (200, 17) and np.isfinite(v).any()
