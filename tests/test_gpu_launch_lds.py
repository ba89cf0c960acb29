"""The dynamic-LDS limit of a kernel is raised once per instantiation and device and follows a high-water mark (csrc/common.h:
launch_lds).  The mark is process-wide state -- inside this pytest process an earlier test may have raised the limit already -- so
the calls run in ONE fresh child process: this file, run as a script.

The child calls ops.gcn_bwd_params at T = 12, V = 25 (launch_gcn_bwd_params<12, 25> -> k_bwd_gcn_params<12, 25>), whose dynamic
LDS follows rows = B * C alone: (2 * min(rows, 32) * 301 + 12 * 25 * 25 + 25 * 12 * 12) * 4 bytes.

    call   x               rows   dynamic LDS
    1      [1,16,12,25]    16      82 928 B   above 64 KB: the limit is raised
    2      [2,16,12,25]    32     121 456 B   above the mark of call 1: raised again (a flag instead of a mark: a launch error)
    3      [1,16,12,25]    16      82 928 B   below the mark: nothing to raise; bit for bit call 1
    4      [1,8,12,25]      8      63 664 B   below 64 KB

Every call returns and matches the fp64 autograd of the oracle's mixing, with the tolerance test_gpu_window.py holds this op to."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [(1, 16), (2, 16), (1, 16), (1, 8)]
T, V = 12, 25


def _child():
    import numpy as np
    import torch
    from coskad_amd import ops
    from oracle import ref_cpu as R
    g = torch.Generator().manual_seed(1225)
    A, Tm = torch.randn(T, V, V, generator=g) * 0.3, torch.randn(V, T, T, generator=g) * 0.3
    data = {shape: (torch.randn(*shape, T, V, generator=g), torch.randn(*shape, T, V, generator=g)) for shape in set(CALLS)}
    got = []
    for i, shape in enumerate(CALLS, 1):
        x, dZ = data[shape]
        dA, dT = ops.gcn_bwd_params(x.cuda(), dZ.cuda(), A.cuda(), Tm.cuda())      # a refused launch raises here
        got.append((dA.cpu(), dT.cpu()))
        A64, T64 = A.double().requires_grad_(True), Tm.double().requires_grad_(True)
        (R.gcn(x.double(), A64, T64) * dZ.double()).sum().backward()
        for name, have, want in (("dA", got[-1][0], A64.grad.float()), ("dT", got[-1][1], T64.grad.float())):
            scale = float(want.abs().max())
            print(f"call {i} {name}: max |error| {float((have - want).abs().max()):.3e}, max |want| {scale:.3e}", flush=True)
            assert torch.isfinite(have).all(), (i, name)
            np.testing.assert_allclose(have.numpy(), want.numpy(), rtol=1e-4, atol=1e-4 * scale, err_msg=f"call {i} {name}")
        print(f"call {i} ok", flush=True)
    assert torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[2][1]), "calls 1 and 3 differ"
    print("calls 1 and 3 equal", flush=True)


@pytest.mark.gpu
def test_lds_limit_follows_the_largest_request():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-3000:]}"
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.endswith(" ok")] == [f"call {i} ok" for i in (1, 2, 3, 4)] and lines[-1] == "calls 1 and 3 equal"


if __name__ == "__main__":
    _child()
