"""Training at the window lengths 8 / 16 / 24 on the stored-Z layer kernels: the default-width one-class step
(STS-GCN 2-32-16-32-64, `linear` projector, latent 16, Euclidean head) at B = 4096 for T in {8, 16, 24} x V in {17, 25} with
`fused_window` on and off, and the passes of one layer on the default stack's layer shapes.

Step rows: {"what": "step", T, V, fused_window, segments, blocks_ms, median_ms}.  Run from a checkout of the PARENT commit (whose
make_train_step has no `fused_window`) the script times that commit's step -- the yardstick: same script, same session, e.g.
    timeout 900 python tools/bench_train_window.py > new.jsonl;  (cd ../parent && timeout 900 python tools/bench_train_window.py --steps-only) > old.jsonl
`fused_window: false` of this build is the cross-check of that figure.  A geometry stays switched on (ops.TRAIN_WINDOW_OFF) only if
its step is more than 3 % faster than the parent's (twice the +-1.5 % box-to-box spread).

Layer rows: {"what": "layer", T, V, Ci, Co, <pass>: {median_us, gbps}} for the statistics pass (in -> Z + moment sums: 2 tensors of
C_in rows), the apply (Z, in -> U: 2 C_in + C_out rows), stage 1 of the backward (dU, Z, in: C_out + 2 C_in rows) and the whole layer
backward (stage 1 + fold + data + parameter kernel; algorithmic bytes: dU, Z, in read, dIn written = C_out + 3 C_in rows), and -- timed
inside that backward by the library's launch probe -- the data pass alone (dU, Z, in -> dZ, dX_res: C_out + 4 C_in rows; C_out + 2 C_in
for the first layer) and the parameter kernel with the sum of its partial rows (in, dZ, dX_res -> dIn: 4 C_in rows; 2 C_in for the first
layer), as us and as GB/s on those algorithmic bytes.  The T = 12 rows run the 12-frame kernels of the same role in the same run
(`--no-12` leaves them out); where the 12-frame backward is one fused kernel the probe sees no data / parameter launch (null).

Every (T, V) runs in a child process of its own under a time limit; the first failure ends the run.  Warm-up first, then the median
of >= 3 timed blocks x 10 calls (HIP events; every block printed).

    timeout 1200 python tools/bench_train_window.py [--batch 4096] [--blocks 3] [--steps 10] [--steps-only | --layers-only]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = (8, 16, 24)
JOINTS = (17, 25)
SHAPES = ((2, 32), (32, 16), (16, 32), (32, 64))       # the default stack


def _time_blocks(fn, warmup: int, blocks: int, steps: int):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def bench_step(T, V, B, fused, warmup, blocks, steps):
    import torch
    from coskad_amd.models.sts.ae import STSE
    from coskad_amd.trainer import make_train_step
    from oracle import ref_cpu as R
    torch.manual_seed(0)
    m = STSE(2, [32, 16, 32], 64, 16, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0).cuda().train()
    m.c.copy_(torch.linspace(-0.2, 0.2, 16))
    kw = dict(lr=1e-4, alpha=1e-6, head='euclidean')
    if fused is not None:
        kw["fused_window"] = fused
    eng = make_train_step(m, **kw)
    x = R.synthetic_clips(B, T=T, V=V, seed=1).cuda()
    t = _time_blocks(lambda: eng.step(x), warmup, blocks, steps)
    return {"what": "step", "T": T, "V": V, "batch": B, "fused_window": fused, "segments": [s.kind for s in eng.stack.segs],
            "blocks_ms": [round(v, 4) for v in t], "median_ms": round(statistics.median(t), 4)}


def bench_layer(T, V, Ci, Co, B, warmup, blocks, steps):
    import torch
    from coskad_amd import engine
    from coskad_amd.models.graph_layers.stsgcn import ST_GCNN_layer, layer_tensors
    from coskad_amd import ops
    torch.manual_seed(T * 100 + V + Ci)
    layer = ST_GCNN_layer(Ci, Co, (1, 1), 1, T, V, 0.0).cuda().train()
    L = layer_tensors(layer)
    first = Ci == 2
    x = torch.randn(B, Ci, T, V, device="cuda")
    slope = None if first else torch.full((1,), 0.25, device="cuda")
    dU = torch.randn(B, Co, T, V, device="cuda") / (B * T * V) ** 0.5
    ws = engine.Workspace()
    u, ctx = engine.chain_forward(x, [L], True, ws, in_slope=slope, want_ctx=True)
    Z, stat = ctx.zs[0], ctx.stats[0]
    wfold, bias, _ = ops.layer_train_stats(x, L.A, L.T, slope, L.w2(L.Wt), L.bt, L.gt, L.bet, L.rm_t, L.rv_t, L.nbt_t, L.w2(L.Wr), L.br,
                                           L.gr, L.ber, L.rm_r, L.rv_r, L.nbt_r, ws.get(ops.train_stats_ws_bytes(Ci), x.device), Z=Z)
    sbuf = ws.get(ops.train_stats_ws_bytes(Ci), x.device)
    bbuf = torch.empty(ops.layer_bwd_ws_bytes(B, Ci, Co, T, V), dtype=torch.uint8, device="cuda")
    grads = {k: torch.zeros_like(v) for k, v in (("A", L.A), ("T", L.T), ("Wt", L.w2(L.Wt)), ("gt", L.gt), ("bet", L.bet))}
    if L.Wr is not None:
        grads.update(Wr=torch.zeros_like(L.w2(L.Wr)), gr=torch.zeros_like(L.gr), ber=torch.zeros_like(L.ber))
    if not first:
        grads["slope_in"] = torch.zeros(1, device="cuda")
    dIn = None if first else torch.empty_like(x)
    row_bytes = 4.0 * B * T * V
    passes = (
        ("stats", lambda: ops.layer_train_moments(x, L.A, L.T, slope, sbuf, Z=Z), 2 * Ci),
        ("apply", lambda: ops.layer_apply_z(Z, x, L.A, L.T, wfold, bias, Co, in_slope=slope, out=u), 2 * Ci + Co),
        ("stage1", lambda: ops.layer_bwd_stats(x, dU, L.A, L.T, slope, L.Wr is not None, bbuf, Z=Z), Co + 2 * Ci),
        ("backward", lambda: ops.layer_bwd(x, dU, L.A, L.T, slope, stat, L.w2(L.Wt), L.gt, L.w2(L.Wr), L.gr, grads, bbuf,
                                           need_dx=not first, dIn=dIn, Z=Z), Co + (2 if first else 3) * Ci),
    )
    row = {"what": "layer", "T": T, "V": V, "Ci": Ci, "Co": Co, "batch": B}
    for name, fn, nrows in passes:
        t = _time_blocks(fn, warmup, blocks, steps)
        med = statistics.median(t)
        row[name] = {"blocks_us": [round(1e3 * v, 1) for v in t], "median_us": round(1e3 * med, 1),
                     "gbps": round(nrows * row_bytes / (med * 1e-3) / 1e9, 1)}
    # single launches inside the backward, by the library's probe (csrc/api.hip): 2 = the data pass, 5 = the parameter kernel
    import ctypes
    from coskad_amd import _lib
    lib, backward = _lib.lib(), passes[3][1]
    for name, kid, nrows in (("data", 2, Co + (2 if first else 4) * Ci), ("params", 5, (2 if first else 4) * Ci)):
        lib.coskad_probe_begin(kid, Ci, Co)
        for _ in range(blocks * steps):
            backward()
        avg, n = ctypes.c_float(0.0), ctypes.c_int(0)
        lib.coskad_probe_end(ctypes.byref(avg), ctypes.byref(n))
        row[name] = ({"launches": n.value, "mean_us": round(1e3 * avg.value, 1), "gbps": round(nrows * row_bytes / (avg.value * 1e-3) / 1e9, 1)}
                     if n.value and avg.value > 0 else None)
    return row


def child(args):
    import torch
    torch.cuda.set_device(0)
    T, V = args.row
    from coskad_amd import trainer
    import inspect
    has_flag = "fused_window" in inspect.signature(trainer.make_train_step).parameters
    if not args.layers_only:
        for fused in ((True, False) if has_flag and T != 12 else (None,)):
            print(json.dumps(bench_step(T, V, args.batch, fused, args.warmup, args.blocks, args.steps)), flush=True)
    if not args.steps_only and has_flag:
        for Ci, Co in SHAPES:
            print(json.dumps(bench_layer(T, V, Ci, Co, args.batch, args.warmup, args.blocks, args.steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--layers-only", action="store_true")
    ap.add_argument("--no-12", action="store_true", help="without the 12-frame rows (the kernels of the same role)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a (T, V) child may take")
    ap.add_argument("--row", type=lambda s: tuple(int(v) for v in s.split(",")), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.blocks >= 3
    if args.row is not None:
        return child(args)
    windows = WINDOWS + (() if args.no_12 else (12,))
    for V in JOINTS:
        for T in windows:
            cmd = [sys.executable, os.path.abspath(__file__), "--row", f"{T},{V}", "--batch", str(args.batch), "--blocks", str(args.blocks),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            cmd += ["--steps-only"] if args.steps_only else []
            cmd += ["--layers-only"] if args.layers_only else []
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"what": "failed", "T": T, "V": V, "rc": rc}), flush=True)
                sys.exit(rc)             # nothing more is started on the GPU after a failure


if __name__ == "__main__":
    main()
