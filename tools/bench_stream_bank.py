"""One tick of C cameras through `StreamBank` against C `StreamScorer.push` calls, on the default 12 x 17 encoder:

  bank       : one `StreamBank.push` of all C cameras, smooth off -- one upload, one push launch, one scoring call, one frames launch
  bank_smooth: the same with smooth on -- plus the smoothing launch (one smoothed score per camera and tick in the steady state)
  scorers    : C `StreamScorer.push` calls, one scorer per camera -- the only way before the bank, and the yardstick

For each C in --cameras: --tracks tracks per camera pushed every frame, `--ticks` timed ticks per route after `--warmup` (which covers
frame 132, from where on every tick smooths), the three routes alternating tick by tick in one process.  Per tick: host = wall time of
the route's calls (enqueue only, nothing synchronises inside), device = the time between two HIP events around them (read after the
calls), both as median and [min, max] over the ticks; `calls` = the library entry points of one tick, counted as tools/bench_stream.py
counts them.  Before timing, the window scores of one tick of `bank` and `scorers` are compared bit for bit.  One JSON row per line.
Exits non-zero without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=300); ap.add_argument("--warmup", type=int, default=140)
    ap.add_argument("--transforms", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_stream_bank: needs the GPU", file=sys.stderr)
        return 2
    if a.ticks < 300:
        ap.error("--ticks: at least 300")
    if a.warmup < 135:
        ap.error("--warmup: at least 135, so that the smoothing launches are in the steady state")
    import yaml
    from coskad_amd import _lib
    from coskad_amd.lit import LitEncoder
    from coskad_amd.stream import StreamBank, StreamScorer
    from coskad_amd.utils.argparser import init_sub_args
    from coskad_amd.utils.dataset import bbox_centre_coordinates, scale_robust
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.load(open(os.path.join(root, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    args, *_ = init_sub_args(Namespace(**dict(cfg, create_experiment_dir=False)))
    torch.manual_seed(0)
    lit = LitEncoder(args).cuda()
    lit.model.eval()
    K, n, res = a.transforms, a.tracks, (1080, 720)
    gen = np.random.default_rng(0)

    def frame_rows(count):
        rows = gen.uniform(50, 600, (count, 34)).astype(np.float32)
        rows[gen.random((count, 34)) < 0.02] = 0.0
        return rows

    _, scaler = scale_robust(bbox_centre_coordinates(frame_rows(4096), np.asarray(res, dtype=np.float32)))
    calls = [0]
    real_call = _lib.call

    def counting_call(*args_, **kw):
        calls[0] += 1
        return real_call(*args_, **kw)

    total = a.warmup + a.ticks + 16
    for C in a.cameras:
        cams = {c: dict(vid_res=res, clip_frames=total) for c in range(C)}
        bank = StreamBank(lit, scaler, cams, max_tracks=C * n, num_transform=K)
        bank_s = StreamBank(lit, scaler, cams, max_tracks=C * n, num_transform=K, smooth=True)
        scorers = [StreamScorer(lit, scaler, res, max_tracks=n, num_transform=K, clip_frames=total) for _ in range(C)]
        ids = list(range(n))
        routes = {"bank": lambda f, rows: bank.push({c: (f, ids, rows[c]) for c in range(C)}),
                  "bank_smooth": lambda f, rows: bank_s.push({c: (f, ids, rows[c]) for c in range(C)}),
                  "scorers": lambda f, rows: [scorers[c].push(f, ids, rows[c]) for c in range(C)]}
        frame = 0
        for _ in range(12):
            frame += 1
            rows = frame_rows(C * n).reshape(C, n, 34)
            got = {name: fn(frame, rows) for name, fn in routes.items()}
        same = torch.equal(got["bank"].window_scores.reshape(K, C, n),
                           torch.stack([o.window_scores for o in got["scorers"]], 1))
        times = {name: ([], []) for name in routes}
        n_calls, smoothed = {}, 0
        _lib.call = sys.modules["coskad_amd.ops"].call = counting_call
        try:
            for it in range(a.warmup + a.ticks):
                frame += 1
                rows = frame_rows(C * n).reshape(C, n, 34)
                for name, fn in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    calls[0] = 0
                    t0 = time.perf_counter()
                    e0.record()
                    out = fn(frame, rows)
                    e1.record()
                    t1 = time.perf_counter()
                    e1.synchronize()
                    n_calls[name] = calls[0]
                    if it >= a.warmup:
                        times[name][0].append((t1 - t0) * 1e3)
                        times[name][1].append(e0.elapsed_time(e1))
                        if name == "bank_smooth":
                            smoothed += sum(c for _, _, c in out.smoothed)
        finally:
            _lib.call = sys.modules["coskad_amd.ops"].call = real_call
        row = {"cameras": C, "tracks_per_camera": n, "transforms": K, "windows_per_tick": C * n * K, "ticks": a.ticks,
               "window_scores_bit_equal": bool(same), "smoothed_per_tick": smoothed / a.ticks}
        for name in times:
            for kind, v in (("host", times[name][0]), ("device", times[name][1])):
                row[f"{name}_{kind}_ms"] = round(statistics.median(v), 4)
                row[f"{name}_{kind}_range_ms"] = [round(min(v), 4), round(max(v), 4)]
            row[f"{name}_calls"] = n_calls[name]
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
