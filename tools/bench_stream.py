"""One `StreamScorer.push` against a host-composed route built from the offline pieces, on the default 12 x 17 encoder:

  stream: coskad_amd.stream.StreamScorer.push -- one pinned upload, the push launch (normalise, ring, windows), the wrapper's eval scoring,
          the frames launch
  host  : per frame bbox_centre_coordinates + scaler.transform (scale_robust) + pose_layout in numpy, a host ring of the last T rows per
          track, the K transformed windows stacked on the host, one pinned upload, the same scoring call.  It stops at the window scores:
          per-person frame scores would need a device -> host copy per push (or the offline ScorePlan once the clip is over).

For each n in --tracks: n tracks pushed every frame (all ready after the first T - 1 frames), `--pushes` timed pushes per route after
`--warmup`, the two routes alternating push by push in one process.  Per push: host = wall time of the call (enqueue only, nothing
synchronises inside), device = the time between two HIP events around it (read after the call); medians over the pushes.  `calls` is the
number of library entry points one push goes through (torch's own kernels, e.g. the upload, are not counted).  Before timing the two
routes' window scores of one frame are compared bit for bit.  One JSON row per line.  Exits non-zero without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace
from collections import deque

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--pushes", type=int, default=300); ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--transforms", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_stream: needs the GPU", file=sys.stderr)
        return 2
    if a.pushes < 200:
        ap.error("--pushes: at least 200")
    import yaml
    from coskad_amd import _lib
    from coskad_amd.lit import LitEncoder
    from coskad_amd.stream import StreamScorer
    from coskad_amd.utils.argparser import init_sub_args
    from coskad_amd.utils.dataset import AE_TRANS_MATS, apply_pose_transform, bbox_centre_coordinates, pose_layout, scale_robust
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.load(open(os.path.join(root, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    args, *_ = init_sub_args(Namespace(**dict(cfg, create_experiment_dir=False)))
    torch.manual_seed(0)
    lit = LitEncoder(args).cuda()
    lit.model.eval()
    T, V, K, res = 12, 17, a.transforms, np.asarray([1080, 720], dtype=np.float32)
    gen = np.random.default_rng(0)

    def frame_rows(n):
        rows = gen.uniform(50, 600, (n, 34)).astype(np.float32)
        rows[gen.random((n, 34)) < 0.02] = 0.0
        return rows

    _, scaler = scale_robust(bbox_centre_coordinates(frame_rows(4096), res))
    calls = [0]
    real_call = _lib.call

    def counting_call(*args_, **kw):
        calls[0] += 1
        return real_call(*args_, **kw)

    def score(x):
        with torch.no_grad():
            return lit.window_scores(lit.model(x))

    for n in a.tracks:
        sc = StreamScorer(lit, scaler, (1080, 720), max_tracks=n, num_transform=K)
        ids = list(range(n))
        rings = [deque(maxlen=T) for _ in range(n)]

        def host_push(rows):
            x, _ = scale_robust(bbox_centre_coordinates(rows, res), scaler)
            fx = np.transpose(pose_layout(x, False, False), (0, 2, 1)).astype(np.float32)          # [n, 3, V]
            for i in range(n):
                rings[i].append(fx[i])
            if len(rings[0]) < T:
                return None
            w = np.stack([np.stack(r, 1) for r in rings])                                              # [n, 3, T, V]
            batch = np.stack([apply_pose_transform(w[i], AE_TRANS_MATS[k])[:2] for k in range(K) for i in range(n)])
            return score(torch.from_numpy(np.ascontiguousarray(batch, dtype=np.float32)).pin_memory().cuda(non_blocking=True))

        frame = 0
        for _ in range(T - 1):                          # fill both routes' rings with the same rows
            frame += 1
            rows = frame_rows(n)
            sc.push(frame, ids, rows)
            host_push(rows)
        frame += 1
        rows = frame_rows(n)
        same = torch.equal(sc.push(frame, ids, rows).window_scores.reshape(-1), host_push(rows).reshape(-1))
        times = {"stream": ([], []), "host": ([], [])}
        n_calls = {}
        _lib.call = sys.modules["coskad_amd.ops"].call = counting_call
        try:
            for it in range(a.warmup + a.pushes):
                frame += 1
                rows = frame_rows(n)
                for name, fn in (("stream", lambda: sc.push(frame, ids, rows)), ("host", lambda: host_push(rows))):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    calls[0] = 0
                    t0 = time.perf_counter()
                    e0.record()
                    fn()
                    e1.record()
                    t1 = time.perf_counter()
                    e1.synchronize()
                    n_calls[name] = calls[0]
                    if it >= a.warmup:
                        times[name][0].append((t1 - t0) * 1e3)
                        times[name][1].append(e0.elapsed_time(e1))
        finally:
            _lib.call = sys.modules["coskad_amd.ops"].call = real_call
        row = {"tracks": n, "transforms": K, "windows_per_push": n * K, "pushes": a.pushes, "window_scores_bit_equal": bool(same)}
        for name in times:
            row[f"{name}_host_ms"] = round(statistics.median(times[name][0]), 4)
            row[f"{name}_device_ms"] = round(statistics.median(times[name][1]), 4)
            row[f"{name}_calls"] = n_calls[name]
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
