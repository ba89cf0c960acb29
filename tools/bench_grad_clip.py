"""What gradient clipping and accumulation cost on the flat train steps: the default 17-joint encoder step (STS-GCN 2-32-16-32-64,
latent 16, Euclidean head) and the default autoencoder step, each with clipping off, with norm clipping on and with accumulate = 2
(per micro-step), at B = 4096 and B = 512.  HIP events; warm-up, then >= 3 blocks of `--steps` steps per setting, the settings
ALTERNATING block by block in one process (the yardstick for "on" is "off" beside it); every block printed, medians compared.

    python tools/bench_grad_clip.py [--batches 4096,512] [--blocks 3] [--steps 20] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = {"off": {}, "norm_clip": {"grad_clip_val": 1.0}, "accumulate2": {"accumulate": 2}}


def _step(model: str, kw):
    from coskad_amd.models.sts.ae import STSAE, STSE
    from coskad_amd.trainer import STSAETrainStep, STSETrainStep
    torch.manual_seed(0)
    if model == "encoder":
        m = STSE(2, [32, 16, 32], 64, 16, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0).cuda().train()
        m.c.copy_(torch.linspace(-0.2, 0.2, 16))
        return STSETrainStep(m, lr=1e-4, alpha=1e-6, head='euclidean', **kw)
    m = STSAE(2, [32, 16, 32], 64, 16, 12, 17, 'sts_gcn', 'linear', 'euclidean', 0.0).cuda().train()
    m.c.copy_(torch.linspace(-0.2, 0.2, 16))
    return STSAETrainStep(m, mode='ae', lr=1e-4, alpha=1e-6, lambda_=0.01, **kw)


def _block(eng, x, steps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.step(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,512")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert args.blocks >= 3 and args.steps % 2 == 0
    torch.cuda.set_device(0)
    from oracle import ref_cpu as R
    for model in ("encoder", "autoencoder"):
        for B in (int(b) for b in args.batches.split(",")):
            x = R.synthetic_clips(B, seed=1).cuda()
            engs = {name: _step(model, kw) for name, kw in SETTINGS.items()}
            for eng in engs.values():
                for _ in range(args.warmup):
                    eng.step(x)
            torch.cuda.synchronize()
            times = {name: [] for name in engs}
            for _ in range(args.blocks):                      # alternating blocks
                for name, eng in engs.items():
                    times[name].append(_block(eng, x, args.steps))
            med = {name: statistics.median(t) for name, t in times.items()}
            for name in engs:
                print(json.dumps({"model": model, "batch": B, "setting": name, "blocks_ms": [round(t, 4) for t in times[name]],
                                  "median_ms": round(med[name], 4), "vs_off_pct": round(100 * (med[name] / med["off"] - 1), 2)}),
                      flush=True)


if __name__ == "__main__":
    main()
