"""CPU checks of the attribution axis (csrc/eval_layer_adj.hip, coskad_amd/attribution.py): the set the adjoint kernel's
predicate states and its host restatement, what the C ABI says before it touches a device, every refusal of
LitEncoder.window_attribution, and the numpy yardstick of the frame maps on a hand-written example.  No kernel runs."""
import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

from coskad_amd import _lib, attribution, ops
from coskad_amd.utils import eval_utils
from coskad_amd.utils.argparser import init_sub_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORTED = {(T, V, Ci, Co) for T in (8, 12, 16, 24) for V in (17, 25) for Ci in (2, 16, 32) for Co in (16, 32, 64)}


def test_predicate_is_the_stated_set_and_ops_restates_it():
    lib = _lib.lib()
    seen = set()
    for T in (8, 10, 12, 16, 24, 32):
        for V in (14, 17, 18, 25, 26):
            for Ci in (1, 2, 4, 8, 16, 32, 64):
                for Co in (2, 8, 16, 32, 48, 64, 128):
                    got = lib.coskad_layer_input_grad_ok(T, V, Ci, Co)
                    assert got in (0, 1)
                    assert bool(got) == ((T, V, Ci, Co) in SUPPORTED), (T, V, Ci, Co)
                    assert ops.layer_input_grad_ok(T, V, Ci, Co) == bool(got), (T, V, Ci, Co)
                    grid = lib.coskad_layer_input_grad_max_grid(T, V, Ci, Co)
                    assert (grid in (256, 512)) if got else grid == 0, (T, V, Ci, Co, grid)
                    assert ops.layer_input_grad_max_grid(T, V, Ci, Co) == grid
                    seen.add((T, V, Ci, Co)) if got else None
    assert seen == SUPPORTED and len(SUPPORTED) == 72


def test_existing_predicates_keep_their_answers():
    lib = _lib.lib()
    for T in (8, 16, 24):
        for V in (17, 25):
            assert lib.coskad_layer_input_grad_ok(T, V, 2, 32) == 1       # the adjoint's set is its own: the forward's has no 2 -> 32
            assert lib.coskad_layer_apply_window_ok(T, V, 2, 32) == 0
            assert lib.coskad_layer_apply_window_ok(T, V, 32, 16) == 1
            assert lib.coskad_layer_tail_ok(T, V, 32, 16) == 0


def _aligned(n_floats):
    """a host buffer and a 16-byte aligned address inside it"""
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_argument_checks_come_before_the_shape_and_the_device():
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    odd = ctypes.c_void_p(a + 4)

    def grad(dU=p, inp=p, dIn=p, A=p, Tm=p, wfold=p, slope=p, B=1, T=8, V=17, Ci=16, Co=16):
        _lib.call("coskad_layer_input_grad_f32", dU, inp, dIn, A, Tm, wfold, slope, B, Ci, Co, T, V, null)

    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`dU` is NULL"):
        grad(dU=null)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`dIn` is NULL"):
        grad(dIn=null)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`in` is NULL"):
        grad(inp=null)                                       # a mask without the tensor it reads
    for name, kw in (("dU", dict(dU=odd)), ("in", dict(inp=odd)), ("dIn", dict(dIn=odd))):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`%s`.*16-byte aligned" % name):
            grad(**kw)
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`%s`.*16-byte aligned" % name):
            grad(V=14, **kw)                                 # the pointer is judged before the shape
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`dU` is NULL"):
        grad(dU=null, T=10, Ci=5)
    for kw in (dict(A=null), dict(Tm=null), dict(wfold=null)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*null pointer"):
            grad(**kw)
    for B in (0, -2):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*B=" + str(B)):
            grad(B=B)
    for kw in (dict(T=10), dict(T=32), dict(V=14), dict(V=18), dict(Ci=8), dict(Ci=64), dict(Co=2), dict(Co=128)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\).*unsupported"):
            grad(**kw)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\).*unsupported"):
        grad(inp=odd, slope=null, V=14)                      # without a mask `in` is not read: only the shape is wrong


def _lit(**over):
    from coskad_amd.lit import LitEncoder
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", "euclidean_encoder.yaml")), Loader=yaml.FullLoader)
    cfg.update(over)
    args, *_ = init_sub_args(Namespace(**cfg))
    return LitEncoder(args)


def _refused(lit, pattern):
    with pytest.raises(ValueError, match=pattern):
        lit.window_attribution(torch.zeros(2, 2, lit.model.n_frames, lit.model.n_joints))


def test_every_refusal_names_its_reason():
    ok = _lit()
    ok.model.eval()
    assert attribution.unsupported_reason(ok) is None
    ok.model.train()
    _refused(ok, "train mode")
    for over, pattern in ((dict(projector="mlp"), "projector 'mlp'"),
                          (dict(encoder_type="Learnable_GCN"), "plain-GCN"),
                          (dict(encoder_type="Static_GCN"), "plain-GCN"),
                          (dict(dataset_headless=True), "V = 14"),
                          (dict(dataset_kp18_format=True), "V = 18"),
                          (dict(channels=[128, 16, 32]), "is wide"),
                          (dict(h_dim=128), "is wide"),
                          (dict(dropout=0.1), "dropout")):
        lit = _lit(**over)
        lit.model.eval()
        assert attribution.unsupported_reason(lit) is not None
        _refused(lit, pattern)
    for T in (8, 16, 24):
        lit = _lit(dataset_seg_len=T)
        lit.model.eval()
        assert attribution.unsupported_reason(lit) is None


def test_decoder_wrappers_are_refused():
    from coskad_amd.lit import LitAutoEncoder, LitVAE
    for cls, name in ((LitAutoEncoder, "euclidean_autoencoder.yaml"), (LitVAE, "spherical_vae.yaml")):
        cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", name)), Loader=yaml.FullLoader)
        args, *_ = init_sub_args(Namespace(**cfg))
        lit = cls(args)
        lit.model.eval()
        with pytest.raises(ValueError, match="autoencoder / VAE"):
            lit.window_attribution(torch.zeros(1, 2, 12, 17))
        with pytest.raises(ValueError, match="autoencoder / VAE"):
            attribution.dataset_attribution(lit, lambda: [], [], "unused")


def test_attribution_frames_on_a_hand_written_example():
    # one clip of 4 frames; person 0 is covered by three 2-frame windows, person 1 by one window over frames 1-2
    gts = {(1, 1): np.zeros(4, dtype=np.int64)}
    trans = torch.zeros(4, dtype=torch.int64)
    meta = torch.tensor([[1, 1, 0, 0], [1, 1, 0, 1], [1, 1, 0, 2], [1, 1, 1, 0]], dtype=torch.int64)
    frames = torch.tensor([[1, 2], [2, 3], [3, 4], [1, 2]], dtype=torch.int32)
    attr = torch.tensor([[[1., 10.], [2., 20.]],
                         [[4., 40.], [8., 80.]],
                         [[16., 160.], [32., 320.]],
                         [[-1., -2.], [-3., -4.]]])
    plan = eval_utils.ScorePlan(trans, meta, frames, gts, 1, device="cpu")
    assert plan.n_persons == 2 and plan.row_ptr.tolist() == [0, 4, 8]
    got = eval_utils.attribution_frames(attr, frames, plan)
    want = np.array([[1., 10.], [3., 30.], [12., 120.], [32., 320.],
                     [-1., -2.], [-3., -4.], [np.nan, np.nan], [np.nan, np.nan]])
    assert got.dtype == np.float64 and got.shape == (8, 2)
    np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError, match="attribution_frames"):
        eval_utils.attribution_frames(attr[:3], frames[:3], plan)
    with pytest.raises(_lib.CoskadHipError, match="no CPU fallback"):
        eval_utils.attribution_frames_device(attr, frames, plan)


def test_save_attribution_writes_one_pair_of_files_per_clip(tmp_path):
    gts = {(1, 1): np.zeros(4, dtype=np.int64), (1, 2): np.zeros(3, dtype=np.int64)}
    trans = torch.tensor([0, 1, 0], dtype=torch.int64)
    meta = torch.tensor([[1, 1, 5, 0], [1, 1, 5, 0], [1, 1, 7, 2]], dtype=torch.int64)
    frames = torch.tensor([[1, 2], [1, 2], [3, 4]], dtype=torch.int32)
    attr = torch.tensor([[[1., 2.], [3., 4.]], [[3., 6.], [5., 8.]], [[9., 9.], [7., 7.]]])
    plan = eval_utils.ScorePlan(trans, meta, frames, gts, 2, device="cpu")
    eval_utils.save_attribution(str(tmp_path), eval_utils.attribution_frames(attr, frames, plan), plan)
    a, p = np.load(tmp_path / "1_1_attribution.npy"), np.load(tmp_path / "1_1_persons.npy")
    assert a.dtype == np.float32 and a.shape == (2, 4, 2) and p.tolist() == [5, 7]
    np.testing.assert_array_equal(a[0], np.array([[2., 4.], [4., 6.], [np.nan] * 2, [np.nan] * 2], dtype=np.float32))   # mean over t
    np.testing.assert_array_equal(a[1], np.array([[np.nan] * 2, [np.nan] * 2, [9., 9.], [7., 7.]], dtype=np.float32))
    assert np.load(tmp_path / "1_2_attribution.npy").shape == (0, 0, 2) and np.load(tmp_path / "1_2_persons.npy").shape == (0,)
