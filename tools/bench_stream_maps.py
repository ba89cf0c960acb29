"""One tick of `StreamBank(maps=True)` against its two yardsticks, on the default 12 x 17 encoder:

  plain   : `StreamBank.push` with maps off -- one upload, one push launch, one scoring call, one frames launch
  map_call: one `lit.window_attribution` call alone, on the windows the plain tick formed
  maps    : `StreamBank.push` with maps on -- plain's launches, the map call, one maps launch

A tick with maps should cost about plain + map_call plus one small launch; `maps_launch_device_ms` is that launch alone, timed by HIP
events around `ops.stream_maps` inside the maps ticks.  For each m in --ready: m tracks of one camera pushed every frame (so m ready
tracks and m x --transforms windows per tick), `--ticks` timed ticks per route after `--warmup`, the routes alternating tick by tick in
one process.  Per tick: host = wall time of the route's calls (enqueue only, nothing synchronises inside), device = the time between
two HIP events around them (read after the calls), both as median and [min, max] over the ticks.  Before timing, the window scores of
one tick of `plain` and `maps` are compared bit for bit.  One JSON row per line.  Exits non-zero without a GPU."""
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
    ap.add_argument("--ready", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--ticks", type=int, default=300); ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--transforms", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_stream_maps: needs the GPU", file=sys.stderr)
        return 2
    if a.ticks < 100:
        ap.error("--ticks: at least 100")
    if a.warmup < 20:
        ap.error("--warmup: at least 20, so that every track has a full window and the allocator is warm")
    import yaml
    from coskad_amd import ops
    from coskad_amd.lit import LitEncoder
    from coskad_amd.stream import StreamBank
    from coskad_amd.utils.argparser import init_sub_args
    from coskad_amd.utils.dataset import bbox_centre_coordinates, scale_robust
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.load(open(os.path.join(root, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    args, *_ = init_sub_args(Namespace(**dict(cfg, create_experiment_dir=False)))
    torch.manual_seed(0)
    lit = LitEncoder(args).cuda()
    lit.model.eval()
    K, res = a.transforms, (1080, 720)
    gen = np.random.default_rng(0)

    def frame_rows(count):
        rows = gen.uniform(50, 600, (count, 34)).astype(np.float32)
        rows[gen.random((count, 34)) < 0.02] = 0.0
        return rows

    _, scaler = scale_robust(bbox_centre_coordinates(frame_rows(4096), np.asarray(res, dtype=np.float32)))
    launch = []
    real_maps = ops.stream_maps

    def timed_maps(*args_, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real_maps(*args_, **kw)
        e1.record()
        launch.append((e0, e1))
        return out

    total = a.warmup + a.ticks + 32
    for m in a.ready:
        cams = {0: dict(vid_res=res, clip_frames=total)}
        plain = StreamBank(lit, scaler, cams, max_tracks=m, num_transform=K)
        maps = StreamBank(lit, scaler, cams, max_tracks=m, num_transform=K, maps=True)
        ids = list(range(m))
        last = {}

        def run_plain(f, rows):
            last["x"] = plain.push({0: (f, ids, rows)})
            return last["x"]

        routes = {"plain": run_plain,
                  "map_call": lambda f, rows: lit.window_attribution(last["x"].windows),
                  "maps": lambda f, rows: maps.push({0: (f, ids, rows)})}
        frame = 0
        for _ in range(14):                                     # every track has a window from frame 12 on
            frame += 1
            rows = frame_rows(m)
            got = {name: fn(frame, rows) for name, fn in routes.items() if name != "map_call" or frame >= plain.R}
        same = torch.equal(got["plain"].window_scores, got["maps"].window_scores) and got["maps"].frame_maps is not None
        times = {name: ([], []) for name in routes}
        launch.clear()
        ops.stream_maps = timed_maps
        try:
            for it in range(a.warmup + a.ticks):
                frame += 1
                rows = frame_rows(m)
                for name, fn in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    fn(frame, rows)
                    e1.record()
                    t1 = time.perf_counter()
                    e1.synchronize()
                    if it >= a.warmup:
                        times[name][0].append((t1 - t0) * 1e3)
                        times[name][1].append(e0.elapsed_time(e1))
        finally:
            ops.stream_maps = real_maps
        row = {"ready_tracks": m, "transforms": K, "windows_per_tick": m * K, "ticks": a.ticks, "window_scores_bit_equal": bool(same),
               "map_state_bytes": ops.stream_maps_state_bytes(m, K, maps.T, maps.V, maps.step)}
        for name in times:
            for kind, v in (("host", times[name][0]), ("device", times[name][1])):
                row[f"{name}_{kind}_ms"] = round(statistics.median(v), 4)
                row[f"{name}_{kind}_range_ms"] = [round(min(v), 4), round(max(v), 4)]
        lv = [e0.elapsed_time(e1) for e0, e1 in launch[a.warmup:]]
        row["maps_launch_device_ms"] = round(statistics.median(lv), 4)
        row["maps_launch_device_range_ms"] = [round(min(lv), 4), round(max(lv), 4)]
        for kind in ("host", "device"):
            row[f"maps_minus_parts_{kind}_ms"] = round(row[f"maps_{kind}_ms"] - row[f"plain_{kind}_ms"] - row[f"map_call_{kind}_ms"], 4)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
