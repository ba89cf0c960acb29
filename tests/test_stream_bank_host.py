"""The camera bank of the online scoring on the CPU (coskad_amd/stream.py `BankPlan` / `StreamBank`, csrc/stream.hip): tracks are keyed
(camera, track id) over one slot pool; every refusal names its reason; the finality watermark and the emission of smoothed scores against a
brute-force restatement on random event sequences; the new entry points refuse bad arguments before they touch a device."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

from coskad_amd import _lib, ops
from coskad_amd.stream import SMOOTH_LAG, BankPlan, StreamBank, emittable
from coskad_amd.utils.argparser import init_sub_args
from coskad_amd.utils.score_plan import RADIUS, gaussian_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = {"a": dict(vid_res=(1080, 720), clip_frames=40), "b": dict(vid_res=(640, 360), clip_frames=30)}


def test_same_track_id_on_two_cameras_is_two_tracks():
    bank = BankPlan(CAMS, 4, 8)
    t = bank.push({"a": (1, [7, 8]), "b": (5, [7])})
    assert t.push.slots == [0, 1, 2] and t.push.reset == [1, 1, 1] and t.cams == ["a", "a", "b"]
    assert bank.plan.slot_of == {("a", 7): 0, ("a", 8): 1, ("b", 7): 2}
    t = bank.push({"b": (6, [7]), "a": (2, [7])})             # each camera has its own frame ids
    assert t.push.slots == [2, 0] and t.push.reset == [0, 0]
    assert list(bank.plan.frames[0]) == [1, 2] and list(bank.plan.frames[2]) == [5, 6]
    for f in range(3, 9):
        t = bank.push({"a": (f, [7]), "b": (f + 4, [7])})
    assert t.push.ready_tracks == [("a", 7), ("b", 7)] and t.push.first_frames == [1, 5] and t.push.out_index == [0, 1]
    assert t.clip_index == [0, 40 + 4]                          # camera b's segment starts at 40


def test_slots_are_reused_after_close_finish_and_reset():
    bank = BankPlan(CAMS, 3, 8)
    bank.push({"a": (1, [1, 2]), "b": (1, [1])})
    with pytest.raises(ValueError, match="4 live tracks, more than max_tracks = 3"):
        bank.push({"a": (2, [1, 2]), "b": (2, [1, 9])})
    assert bank.cams["a"].last == 1 and bank.cams["b"].last == 1        # the refused push changed nothing
    t = bank.close("a", [1])
    assert [(c.track, c.slot, c.rows) for c in t.closed] == [(("a", 1), 0, [(0, 1)])] and t.close_clip == [0]
    assert bank.push({"b": (2, [1, 9])}).push.slots == [2, 0]
    t = bank.finish("b")
    assert sorted(c.slot for c in t.closed) == [0, 2] and bank.plan.live == [("a", 2)]
    assert bank.push({"a": (2, [2, 5, 6])}).push.slots == [1, 0, 2]
    assert bank.reset("a") is False and bank.plan.live == [] and bank.cams["a"].last == 0
    assert bank.push({"a": (1, [2])}).push.slots == [0]
    assert bank.reset("b", clip_frames=50) is True and bank.total == 90 and bank.cams["b"].finished is None
    assert bank.reset("a", clip_frames=10) is True and bank.cams["b"].offset == 10 and bank.clip_index("b", 50) == 59
    assert bank.clip_index("a", 11) == -1 and bank.clip_index("a", 0) == -1 and bank.clip_index("a", 10) == 9


def test_refusals_name_their_reason():
    bank = BankPlan(CAMS, 2, 8)
    with pytest.raises(ValueError, match="unknown camera 'c'"):
        bank.push({"c": (1, [1])})
    bank.push({"a": (3, [1])})
    for f in (3, 2):
        with pytest.raises(ValueError, match=f"frame id {f} does not increase on camera 'a' \\(its last frame is 3\\)"):
            bank.push({"a": (f, [1])})
    with pytest.raises(ValueError, match="3 live tracks, more than max_tracks = 2"):
        bank.push({"a": (4, [1, 2]), "b": (1, [1])})
    with pytest.raises(ValueError, match="duplicate track id 4 on camera 'b'"):
        bank.push({"b": (1, [4, 4])})
    with pytest.raises(ValueError, match="track 9 is not live on camera 'a'"):
        bank.close("a", [9])
    with pytest.raises(ValueError, match="n_frames = 2 on camera 'a'"):
        bank.finish("a", 2)                                     # frame 3 was pushed
    bank.finish("a", 3)
    with pytest.raises(ValueError, match="push after finish: camera 'a'"):
        bank.push({"a": (4, [1])})
    with pytest.raises(ValueError, match="finished its clip already"):
        bank.finish("a")
    bank.reset("a")
    bank.push({"a": (1, [1])})
    with pytest.raises(ValueError, match="smooth = True needs clip_frames on every camera; camera 'b' has none"):
        BankPlan({"a": dict(vid_res=(8, 8), clip_frames=5), "b": dict(vid_res=(8, 8))}, 2, 8, smooth=True)
    with pytest.raises(ValueError, match="unknown setting 'fps'"):
        BankPlan({"a": dict(vid_res=(8, 8), fps=25)}, 2, 8)
    with pytest.raises(ValueError, match="vid_res = None .* and cameras with a resolution in one bank"):
        BankPlan({"a": dict(vid_res=(8, 8)), "b": dict(vid_res=None)}, 2, 8)
    with pytest.raises(ValueError, match="unsupported window of 10 frames"):
        BankPlan(CAMS, 2, 10)


def _lit(cls_name, yaml_name, **over):
    from coskad_amd import lit as L
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", yaml_name)), Loader=yaml.FullLoader)
    cfg.update(over)
    args, *_ = init_sub_args(Namespace(**cfg))
    return getattr(L, cls_name)(args)


def test_bank_refusals_are_the_scorers():
    lit = _lit("LitEncoder", "euclidean_encoder.yaml")
    lit.model.train()
    with pytest.raises(ValueError, match="StreamBank: the model is in train mode"):
        StreamBank(lit, None, CAMS)
    vae = _lit("LitVAE", "spherical_vae.yaml")
    vae.model.eval()
    with pytest.raises(ValueError, match="StreamBank: LitVAE.*SAMPLED latent"):
        StreamBank(vae, None, CAMS)
    lit3 = _lit("LitEncoder", "euclidean_encoder.yaml", num_coords=3)
    lit3.model.eval()
    with pytest.raises(ValueError, match="StreamBank: num_coords = 3"):
        StreamBank(lit3, None, CAMS)
    lit.model.eval()
    with pytest.raises(ValueError, match="smooth = True needs clip_frames on every camera; camera 'x' has none"):
        StreamBank(lit, None, {"x": dict(vid_res=(1080, 720))}, smooth=True)


# ---- watermark and emission against a brute-force restatement ----------------------------------------------------------------------

class _Brute:
    """One camera, restated: a frame is final when its id <= the camera's last pushed id and every track with a row at it has had
    R - 1 further rows or is closed; the watermark is the number of leading final frames, at most clip_frames."""

    def __init__(self, R, n):
        self.R, self.n, self.last, self.rows, self.closed = R, n, 0, {}, set()

    def final(self, f):
        if f > self.last:
            return False
        for key, fr in self.rows.items():
            if f in fr and key not in self.closed and len(fr) - 1 - fr.index(f) < self.R - 1:
                return False
        return True

    def watermark(self):
        w = 0
        while w < self.n and self.final(w + 1):
            w += 1
        return w


@pytest.mark.parametrize("seed,T,stride,idle", [(0, 8, 1, 4), (1, 8, 1, None), (2, 12, 1, 6), (3, 8, 3, 30)])
def test_watermark_and_emission_against_a_brute_force_restatement(seed, T, stride, idle):
    gen = np.random.default_rng(seed)
    n = {"a": 420, "b": 150}                                    # camera a ends inside its clip vector, camera b is pushed past its own
    bank = BankPlan({c: dict(vid_res=(1080, 720), clip_frames=n[c]) for c in n}, 12, T, stride, smooth=True, idle_close=idle)
    R = bank.plan.R
    brute = {c: _Brute(R, n[c]) for c in n}
    live = {c: {} for c in n}                                   # track id -> (incarnation, last seen)
    serial = {c: 0 for c in n}
    emitted = {c: [] for c in n}
    early = 0

    def check(tick, cams):
        nonlocal early
        for c in cams:
            assert bank.watermark(c) == brute[c].watermark(), c
        for c, first, count in tick.smoothed:
            assert count > 0 and first == len(emitted[c]), (c, first)          # contiguous, every index once
            w = brute[c].watermark()
            if bank.cams[c].finished is None:
                assert all(w >= i + 121 for i in range(first, first + count)), (c, first, count, w)
                early += count
            emitted[c] += list(range(first, first + count))
        rows = [(bank.cams[c].offset, bank.cams[c].n if bank.cams[c].finished is None else bank.cams[c].finished, i)
                for c, first, count in tick.smoothed for i in range(first, first + count)]
        assert tick.items == rows

    frame = {c: 0 for c in n}
    for _ in range(300):
        batch = {}
        for c in n:
            if gen.random() < 0.1:
                continue                                        # the camera sits this tick out
            frame[c] += 1 if gen.random() < 0.9 else int(gen.integers(2, 5))    # cameras skip frame ids
            f = frame[c]
            if idle is not None:                                # the bank's rule, restated: not seen for more than `idle` frame ids
                for t in [t for t, (_, seen) in live[c].items() if f - seen > idle]:
                    brute[c].closed.add((t, live[c].pop(t)[0]))
            if len(live[c]) < 5 and gen.random() < 0.15:        # tracks start late
                serial[c] += 1
                fresh = int(gen.integers(0, 4)) * 100 + serial[c]
                live[c][fresh] = (serial[c], f)
            else:
                fresh = None
            here = [t for t in live[c] if t == fresh or gen.random() < 0.8]     # and skip frames, or go idle for a while
            for t in here:
                live[c][t] = (live[c][t][0], f)
                brute[c].rows.setdefault((t, live[c][t][0]), []).append(f)
            brute[c].last = f
            batch[c] = (f, here)
        if batch:
            check(bank.push(batch), list(batch))
        for c in n:                                             # tracks close early
            if live[c] and gen.random() < 0.03:
                t = list(live[c])[int(gen.integers(len(live[c])))]
                brute[c].closed.add((t, live[c].pop(t)[0]))
                check(bank.close(c, [t]), [c])
    assert frame["a"] + 3 < n["a"] and frame["b"] > n["b"] and early > 0 and bank.watermark("b") <= n["b"]
    for c in n:
        before = len(emitted[c])
        end = n[c] if c == "b" else frame[c] + 3
        tick = bank.finish(c, end)
        assert bank.plan.live == [k for k in bank.plan.live if k[0] != c]
        check(tick, [])
        assert emitted[c] == list(range(end)) and before < end
        assert all(o == bank.cams[c].offset and m == end for o, m, _ in tick.items)


def test_emission_rule():
    assert SMOOTH_LAG == RADIUS == 120 and len(gaussian_taps()) == SMOOTH_LAG + 1
    assert [emittable(w) for w in (0, 1, 120, 121, 122, 250)] == [0, 0, 0, 1, 2, 130]
    bank = BankPlan({"a": dict(vid_res=None, clip_frames=400)}, 2, 8, smooth=True)
    got = []
    for f in range(1, 131):
        t = bank.push({"a": (f, [])})                           # a frame that shows nobody still moves the watermark
        assert bank.watermark("a") == f and t.push is None
        got += t.smoothed
    assert got == [("a", i, 1) for i in range(10)]
    t = bank.push({"a": (131, [1])})
    assert bank.watermark("a") == 130 and t.smoothed == []      # the new track's only row is not final
    t = bank.push({"a": (140, [])})
    assert bank.watermark("a") == 130
    t = bank.close("a")
    assert bank.watermark("a") == 140 and t.smoothed == [("a", 10, 10)]
    assert bank.finish("a", 150).smoothed == [("a", 20, 130)]


# ---- the library ----------------------------------------------------------------------------------------------------------------

def test_host_predicates_agree_with_the_library():
    lib = _lib.lib()
    assert lib.coskad_stream_smooth_lag() == SMOOTH_LAG
    for T in (8, 10, 12, 16, 24, 32):
        for V in (14, 16, 17, 18):
            assert bool(lib.coskad_stream_ok(T, V)) == ops.stream_ok(T, V)
            if ops.stream_ok(T, V):
                assert BankPlan(CAMS, 2, T, 2).plan.R == ops.stream_rows(T, 2)


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    null = None
    buf = (ctypes.c_double * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    slots = (ctypes.c_int * 4)(0, 1, 2, 3)
    res = (ctypes.c_float * 8)(1080, 720, 640, 360, 1080, 720, 1, 1)
    Err = _lib.CoskadHipError

    def push(raw=p, slot=p, slot_host=slots, reset=p, out_index=p, center=p, scale=p, res=p, res_host=res, flags=0, mats=p, ring=p,
             count=p, x_out=p, n=4, m=2, M=4, K=5, T=12, V=17, step=1):
        _lib.call("coskad_stream_push_cams_f32", raw, slot, slot_host, reset, out_index, center, scale, res, res_host, flags, mats, ring,
                  count, x_out, n, m, M, K, T, V, step, null)

    for name in ("raw", "slot", "slot_host", "reset", "out_index", "mats", "ring", "count", "x_out"):
        with pytest.raises(Err, match=r"\(-1\): stream_push_cams: null pointer"):
            push(**{name: null})
    for name in ("res", "res_host"):
        with pytest.raises(Err, match=r"\(-1\): stream_push_cams: null pointer \(res\)"):
            push(**{name: null})
    with pytest.raises(Err, match=r"\(-1\): stream_push_cams: center and scale come together"):
        push(center=null)
    for kw in (dict(n=0), dict(m=5), dict(M=0), dict(K=0), dict(step=0)):
        with pytest.raises(Err, match=r"\(-1\): stream_push_cams: n="):
            push(**kw)
    for kw in (dict(T=10), dict(V=16)):
        with pytest.raises(Err, match=r"\(-2\): stream_push_cams: unsupported"):
            push(**kw)
    with pytest.raises(Err, match=r"\(-1\): stream_push_cams: n_joints=14 with layout flags 1"):
        push(V=14, flags=1)
    with pytest.raises(Err, match=r"\(-1\): stream_push_cams: res\[2\]: video resolution 0 x 720"):
        push(res_host=(ctypes.c_float * 8)(1080, 720, 640, 360, 0, 720, 1, 1))
    with pytest.raises(Err, match=r"\(-1\): stream_push_cams: res\[1\]: video resolution 640 x nan"):
        push(res_host=(ctypes.c_float * 8)(1080, 720, 640, float("nan"), 1, 1, 1, 1))
    with pytest.raises(Err, match=r"\(-1\): stream_push_cams: a slot outside \[0, max_tracks\)"):
        push(slot_host=(ctypes.c_int * 4)(0, 1, 2, 4))
    with pytest.raises(Err, match=r"\(-1\): stream_push_cams: a slot twice in one launch"):
        push(slot_host=(ctypes.c_int * 4)(0, 1, 1, 3))

    items = (ctypes.c_int * 9)(0, 37, 0, 37, 121, 120, 158, 400, 399)

    def smooth(clip=p, items=p, items_host=items, taps=p, n_taps=121, per_t=p, mean=p, n_items=3, K=2, F=558):
        _lib.call("coskad_stream_smooth_f64", clip, items, items_host, taps, n_taps, per_t, mean, n_items, K, F, null)

    for name, what in (("clip", "clip"), ("items", "items"), ("items_host", "items"), ("taps", "taps"), ("per_t", "per_t, mean"),
                       ("mean", "per_t, mean")):
        with pytest.raises(Err, match=rf"\(-1\): stream_smooth: null pointer \({what}\)"):
            smooth(**{name: null})
    for kw in (dict(n_items=0), dict(K=0), dict(F=0), dict(n_items=-1)):
        with pytest.raises(Err, match=r"\(-1\): stream_smooth: n_items="):
            smooth(**kw)
    for taps in (120, 122, 241):
        with pytest.raises(Err, match=rf"\(-2\): stream_smooth: unsupported tap table of {taps} entries: the filter has 121 taps"):
            smooth(n_taps=taps)
    with pytest.raises(Err, match=r"\(-1\): stream_smooth: items\[2\] = \(offset 158, n 400, index 399\) outside the buffer of 557 frames"):
        smooth(F=557)
    for row, bad in ((0, (-1, 37, 0)), (1, (37, 121, 121)), (1, (37, 0, 0)), (2, (158, 400, -1)), (0, (2 ** 31 - 1, 2 ** 31 - 1, 0))):
        table = list(items)
        table[3 * row:3 * row + 3] = bad
        with pytest.raises(Err, match=rf"\(-1\): stream_smooth: items\[{row}\] = \(offset {bad[0]}, n {bad[1]}, index {bad[2]}\) outside"):
            smooth(items_host=(ctypes.c_int * 9)(*table))


def test_new_wrappers_have_no_cpu_fallback():
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.stream_push_cams(torch.zeros(1, 34), i32(1), i32(1), i32(1), i32(1), None, None, torch.ones(1, 2), torch.ones(2), 0,
                             torch.zeros(1, 3, 3), torch.zeros(2, 12, 2, 17), i32(2), 0, 12, 17, 1)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.stream_smooth(torch.zeros(2, 8, dtype=torch.float64), i32(3).view(1, 3), i32(3), torch.zeros(121, dtype=torch.float64))
