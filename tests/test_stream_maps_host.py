"""Per-joint maps of the stream on the CPU (coskad_amd/stream.py, csrc/stream.hip): `maps=True` refuses what the wrapper's
own map call refuses, with that call's reason, and `maps=False` keeps accepting it; the maps entry points refuse bad arguments before
they touch a device; ops.stream_maps_state_bytes restates the library's size query."""
import ctypes
import os
from argparse import Namespace

import pytest
import torch
import yaml

from coskad_amd import _lib, ops
from coskad_amd.stream import BankOut, StreamBank, StreamOut, StreamScorer
from coskad_amd.utils.argparser import init_sub_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lit(cls_name, yaml_name, **over):
    from coskad_amd import lit as L
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", yaml_name)), Loader=yaml.FullLoader)
    cfg.update(over)
    args, *_ = init_sub_args(Namespace(**cfg))
    lit = getattr(L, cls_name)(args)
    lit.model.eval()
    return lit


def _accepted_up_to_the_device(build):
    """`maps=False` takes the wrapper: construction gets past every refusal (each a ValueError) and as far as its pinned staging buffers,
    which torch cannot give without a GPU (RuntimeError)"""
    try:
        build()
    except ValueError as e:
        pytest.fail(f"maps=False refused the wrapper: {e}")
    except RuntimeError as e:
        assert "GPU" in str(e) or "pin" in str(e).lower() or "CUDA" in str(e), e


def test_refusals_name_their_reason():
    from coskad_amd import attribution
    cams = {0: dict(vid_res=(1080, 720), clip_frames=None)}
    mlp = _lit("LitEncoder", "euclidean_encoder.yaml", projector="mlp")
    headless = _lit("LitEncoder", "euclidean_encoder.yaml", dataset_headless=True)
    for lit, reason in ((mlp, "projector 'mlp'"), (headless, "V = 14")):
        why = attribution.unsupported_reason(lit)
        assert why is not None and reason in why
        with pytest.raises(ValueError, match=reason) as e:
            StreamScorer(lit, None, (1080, 720), maps=True)
        assert why in str(e.value) and "maps = True" in str(e.value)          # the wrapper's reason, verbatim
        with pytest.raises(ValueError, match=reason) as e:
            StreamBank(lit, None, cams, maps=True)
        assert why in str(e.value)
        _accepted_up_to_the_device(lambda: StreamScorer(lit, None, (1080, 720), maps=False))
        _accepted_up_to_the_device(lambda: StreamScorer(lit, None, (1080, 720)))
    train = _lit("LitEncoder", "euclidean_encoder.yaml")
    train.model.train()
    for maps in (True, False):                                               # refused with and without maps, as today
        with pytest.raises(ValueError, match="train mode"):
            StreamScorer(train, None, (1080, 720), maps=maps)
    ae = _lit("LitAutoEncoder", "euclidean_autoencoder.yaml")
    ae.score_type = 'hyp'
    with pytest.raises(ValueError, match="score type 'hyp' has no reconstruction term") as e:
        StreamScorer(ae, None, (1080, 720), maps=True)
    assert ae._error_map_refusal() in str(e.value)
    with pytest.raises(ValueError, match="score type 'hyp' has no reconstruction term"):
        StreamBank(ae, None, cams, maps=True)
    _accepted_up_to_the_device(lambda: StreamScorer(ae, None, (1080, 720), maps=False))


def test_outputs_carry_the_map_fields_last_and_empty_by_default():
    for cls in (StreamOut, BankOut):
        assert cls._fields[-2:] == ("frame_maps", "window_maps")
        out = cls([], [], None, [], None)
        assert out.frame_maps is None and out.window_maps is None
    assert StreamOut._fields[:6] == ("tracks", "first_frames", "window_scores", "final", "frame_scores", "windows")
    assert BankOut._fields[:9] == ("tracks", "first_frames", "window_scores", "final", "frame_scores", "windows", "smoothed",
                                   "smoothed_scores", "smoothed_mean")


def test_size_query_agrees_with_the_library():
    lib = _lib.lib()
    protos = _lib.prototypes()
    assert protos["coskad_stream_maps_state_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert len(protos["coskad_stream_maps_f64"][1]) == 14 and len(protos["coskad_stream_maps_close_f64"][1]) == 14
    for M in (1, 6, 257):
        for K in (1, 2, 5):
            for T in (8, 10, 12, 16, 24):
                for V in (14, 17, 18, 25):
                    for step in (1, 3):
                        want = lib.coskad_stream_maps_state_bytes(M, K, T, V, step)
                        assert ops.stream_maps_state_bytes(M, K, T, V, step) == want, (M, K, T, V, step)
                        assert (want == 0) == (not ops.stream_ok(T, V))
    # running sums and counts per (track, transformation, ring row, joint): O(M K R V), not the windows themselves
    assert ops.stream_maps_state_bytes(6, 2, 12, 17, 1) == 6 * 2 * 12 * 17 * 8 + 6 * 2 * 12 * 4
    assert ops.stream_maps_state_bytes(1, 1, 8, 14, 3) == 22 * 14 * 8 + 22 * 4
    assert ops.stream_maps_state_bytes(1, 1, 8, 17, 1) == 8 * 17 * 8 + 8 * 4
    assert ops.stream_maps_state_bytes(1, 3, 8, 17, 1) % 8 == 0 and ops.stream_maps_state_bytes(1, 3, 8, 17, 1) == 24 * 17 * 8 + 96
    assert ops.stream_maps_state_bytes(1, 1, 24, 17, 3) % 8 == 0          # 70 counts: 280 bytes, rounded up to 8
    for bad in ((0, 1, 12, 17, 1), (1, 0, 12, 17, 1), (1, 1, 12, 17, 0), (1, 1, 12, 17, 2 ** 27)):
        assert ops.stream_maps_state_bytes(*bad) == 0 == lib.coskad_stream_maps_state_bytes(*bad)
    with pytest.raises(ValueError, match="stream_maps_state: unsupported"):
        ops.stream_maps_state(4, 2, 10, 17, 1, "cpu")


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    null = None
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    slots = (ctypes.c_int * 4)(0, 1, 2, 3)
    Err = _lib.CoskadHipError
    need = ops.stream_maps_state_bytes(4, 2, 12, 17, 1)
    assert need <= ctypes.sizeof(buf)

    def maps(maps=p, slot=p, slot_host=slots, count=p, state=p, state_bytes=need, out=p, m=4, M=4, K=2, T=12, V=17, step=1):
        _lib.call("coskad_stream_maps_f64", maps, slot, slot_host, count, state, state_bytes, out, m, M, K, T, V, step, null)

    for name in ("maps", "slot", "slot_host", "count", "state", "out"):
        with pytest.raises(Err, match=r"\(-1\): stream_maps: null pointer"):
            maps(**{name: null})
    with pytest.raises(Err, match=r"\(-1\): stream_maps: m=5 ready tracks, more than max_tracks=4"):
        maps(m=5)
    for kw in (dict(m=0), dict(m=-2), dict(K=0), dict(step=0)):
        with pytest.raises(Err, match=r"\(-1\): stream_maps: m="):
            maps(**kw)
    for kw in (dict(T=10), dict(V=25), dict(T=32), dict(V=16)):
        with pytest.raises(Err, match=r"\(-2\): stream_maps: unsupported \(n_frames="):
            maps(**kw)
    for bad in ((0, 1, 2, 4), (0, -1, 2, 3)):
        with pytest.raises(Err, match=r"\(-1\): stream_maps: a slot outside \[0, max_tracks\)"):
            maps(slot_host=(ctypes.c_int * 4)(*bad))
    with pytest.raises(Err, match=r"\(-1\): stream_maps: a slot twice in one launch"):
        maps(slot_host=(ctypes.c_int * 4)(0, 1, 1, 3))
    with pytest.raises(Err, match=rf"\(-1\): stream_maps: state of {need - 8} bytes, coskad_stream_maps_state_bytes asks for {need}"):
        maps(state_bytes=need - 8)
    with pytest.raises(Err, match=r"\(-1\): stream_maps: state of \d+ bytes"):
        maps(step=3)                                             # the same buffer is too small for a ring of 34 rows
    with pytest.raises(Err, match=r"\(-1\): stream_maps: state is not aligned to 8 bytes"):
        maps(state=ctypes.c_void_p(p.value + 4))

    def close(row_slot=p, row_slot_host=slots, row_index=p, count=p, state=p, state_bytes=need, out=p, rows=4, M=4, K=2, T=12, V=17,
              step=1):
        _lib.call("coskad_stream_maps_close_f64", row_slot, row_slot_host, row_index, count, state, state_bytes, out, rows, M, K, T, V,
                  step, null)

    for name in ("row_slot", "row_slot_host", "row_index", "count", "state", "out"):
        with pytest.raises(Err, match=r"\(-1\): stream_maps_close: null pointer"):
            close(**{name: null})
    for kw in (dict(rows=0), dict(K=0), dict(step=-1)):
        with pytest.raises(Err, match=r"\(-1\): stream_maps_close: rows="):
            close(**kw)
    for kw in (dict(T=10), dict(V=25)):
        with pytest.raises(Err, match=r"\(-2\): stream_maps_close: unsupported \(n_frames="):
            close(**kw)
    for bad in ((0, 1, 2, 4), (0, -1, 2, 3)):
        with pytest.raises(Err, match=r"\(-1\): stream_maps_close: a slot outside \[0, max_tracks\)"):
            close(row_slot_host=(ctypes.c_int * 4)(*bad))
    with pytest.raises(Err, match=r"\(-1\): stream_maps_close: state of \d+ bytes, coskad_stream_maps_state_bytes asks for"):
        close(state_bytes=need - 1)


def test_wrappers_have_no_cpu_fallback():
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    state = torch.zeros(ops.stream_maps_state_bytes(2, 1, 12, 17, 1) // 8, dtype=torch.float64)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.stream_maps(torch.zeros(1, 12, 17), i32(1), i32(1), i32(2), state, 1, 12, 17, 1)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        ops.stream_maps_close(i32(1), i32(1), i32(1), i32(2), state, 1, 12, 17, 1)
