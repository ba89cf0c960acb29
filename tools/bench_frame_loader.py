"""Batch formation from the two device residencies of the robust pipeline, on synthetic trajectories built on the device (no CSVs):

  windows: DeviceWindows' table xy [N, 2, T V] + coskad_gather_transform_f32     (`dataset_resident: 'windows'`, the yardstick)
  frames : FrameWindows' table fxy [F, 2, V] + win_row [N] + coskad_gather_frames_f32     (`dataset_resident: 'frames'`)

Sizes: `--size ubnormal` takes the 1.76 M rows of tools/bench_score_device.py's table (200 clips x 4 persons x 5 x 439 starts) as the
windows of 4000 trajectories of 450 frames; `--size small` is 200 such trajectories, where both tables fit the last-level cache.
For each B in --batches and for shuffled and sequential indices: `--blocks` timed blocks of `--iters` launches each between two HIP
events, after `--warmup` untimed blocks; the two routes alternate block by block and every block is printed; each launch of a block
gets its own index batch.  Before any time is printed the two routes' outputs are compared bit for bit.
GB/s = (bytes written + bytes the batch must read: its distinct table rows, its indices) / median time.
One JSON row per line.  Exits non-zero without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"ubnormal": 4000, "small": 200}


def build_tables(n_traj, n_frames, T, V, step, seed=0):
    """fxy [F, 2, V], win_row [N] int32, xy [N, 2, T V] (the same values, one copy per window), all on the device"""
    gen = torch.Generator("cuda").manual_seed(seed)
    F, span = n_traj * n_frames, (T - 1) * step
    fxy = torch.randn(F, 2, V, device="cuda", generator=gen)
    starts = torch.arange(n_frames - span, device="cuda")
    win_row = (torch.arange(n_traj, device="cuda")[:, None] * n_frames + starts[None]).reshape(-1).to(torch.int32)
    N = win_row.numel()
    xy = torch.empty(N, 2, T * V, device="cuda")
    off = step * torch.arange(T, device="cuda")
    for i in range(0, N, 1 << 16):                                   # in pieces: the temporary stays small
        rows = win_row[i:i + (1 << 16)].long()[:, None] + off        # [n, T]
        xy[i:i + (1 << 16)] = fxy[rows].permute(0, 2, 1, 3).reshape(-1, 2, T * V)
    return fxy, win_row, xy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES), default="ubnormal"); ap.add_argument("--frames", type=int, default=450)
    ap.add_argument("--seg-len", type=int, default=12); ap.add_argument("--joints", type=int, default=17)
    ap.add_argument("--stride", type=int, default=1); ap.add_argument("--transforms", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--blocks", type=int, default=7); ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--orders", nargs="+", choices=["shuffled", "sequential"], default=["shuffled", "sequential"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_frame_loader: needs the GPU", file=sys.stderr)
        return 2
    if a.blocks < 5:
        ap.error("--blocks: at least 5")
    from coskad_amd import ops
    from coskad_amd.utils.dataset import AE_TRANS_MATS
    T, V, step = a.seg_len, a.joints, a.stride
    fxy, win_row, xy = build_tables(SIZES[a.size], a.frames, T, V, step)
    mats = torch.from_numpy(AE_TRANS_MATS[:a.transforms].copy()).cuda()
    N, F = win_row.numel(), fxy.shape[0]
    n_items = N * a.transforms
    print(json.dumps({"what": "tables", "size": a.size, "windows": N, "frame_rows": F, "T": T, "V": V, "step": step,
                      "window_table_bytes": xy.numel() * 4, "frame_table_bytes": fxy.numel() * 4 + win_row.numel() * 4,
                      "of_which_win_row_bytes": win_row.numel() * 4}))

    routes = {"windows": lambda idx: ops.gather_transform(xy, mats, idx, T, V),
              "frames": lambda idx: ops.gather_frames(fxy, win_row, mats, idx, T, V, step)}
    gen = torch.Generator("cuda").manual_seed(1)
    for B in a.batches:
        for order in a.orders:
            if order == "shuffled":
                pool = torch.randint(0, n_items, (a.iters, B), device="cuda", generator=gen)
            else:                                                     # consecutive items, each launch further along the table
                first = torch.arange(a.iters, device="cuda") * (n_items // a.iters)
                pool = (first[:, None] + torch.arange(B, device="cuda")[None]) % n_items
            for k in (0, a.iters - 1):                               # the routes agree, or no time is printed
                assert torch.equal(routes["windows"](pool[k]), routes["frames"](pool[k])), (B, order, k)
            rows0 = (win_row[pool[0] % N].long()[:, None] + step * torch.arange(T, device="cuda")).unique().numel()
            wins0 = (pool[0] % N).unique().numel()
            written = B * 2 * T * V * 4
            must = {"windows": written + wins0 * 2 * T * V * 4 + B * 8,
                    "frames": written + rows0 * 2 * V * 4 + B * 8 + wins0 * 4}
            ms = {r: [] for r in routes}
            for blk in range(a.warmup + a.blocks):
                for r, fn in routes.items():                         # alternate inside one block index
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for k in range(a.iters):
                        fn(pool[k])
                    e1.record()
                    e1.synchronize()
                    if blk >= a.warmup:
                        ms[r].append(e0.elapsed_time(e1) / a.iters)
            for r in routes:
                med = statistics.median(ms[r])
                print(json.dumps({"what": "gather", "route": r, "size": a.size, "B": B, "order": order,
                                  "median_us": round(med * 1e3, 2), "blocks_us": [round(v * 1e3, 2) for v in ms[r]],
                                  "iters_per_block": a.iters, "must_move_bytes": must[r],
                                  "GBps": round(must[r] / (med * 1e-3) / 1e9, 1)}))
            mw, mf = statistics.median(ms["windows"]), statistics.median(ms["frames"])
            print(json.dumps({"what": "ratio", "size": a.size, "B": B, "order": order, "frames_over_windows": round(mf / mw, 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
