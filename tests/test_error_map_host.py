"""CPU checks of the reconstruction-error maps: what the new entry point says before it touches a device, that the header
declares it and ops binds it, every refusal of the wrappers' window_error_map / window_latent_attribution, the split of
attribution.unsupported_reason, the map formula of the route without the tail kernel and save_attribution's file names.  No kernel runs."""
import ctypes
import inspect
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch
import yaml

from coskad_amd import _lib, attribution, ops
from coskad_amd.utils import eval_utils
from coskad_amd.utils.argparser import init_sub_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the entry point ------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_and_ops_binds_it():
    assert "coskad_layer_tail_map_f32" in _lib.header_symbols()
    assert hasattr(_lib.lib(), "coskad_layer_tail_map_f32")
    assert _lib.lib().coskad_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "coskad_hip.h")).read()
    proto = re.search(r"int coskad_layer_tail_map_f32\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == 17
    src = inspect.getsource(ops.layer_tail_map)
    site = re.search(r'call\("coskad_layer_tail_map_f32",(.*?)tag=', src, flags=re.S).group(1)
    assert len([a for a in site.split(",") if a.strip()]) == 17
    assert len(inspect.signature(ops.layer_tail).parameters) == 13       # layer_tail keeps its signature


def _aligned(n_floats):
    """a host buffer and a 16-byte aligned address inside it"""
    buf = (ctypes.c_float * (n_floats + 8))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_argument_checks_come_before_the_device():
    null = ctypes.c_void_p(0)
    buf, a = _aligned(64)
    p = ctypes.c_void_p(a)
    odd = ctypes.c_void_p(a + 4)

    def tail(inp=p, x=p, out=p, score=p, emap=p, A=p, wfold=p, B=1, T=8, V=17, Ci=32, Co=2):
        _lib.call("coskad_layer_tail_map_f32", inp, x, out, score, emap, A, p, wfold, p, null, null, B, Ci, Co, T, V, null)

    for kw in (dict(inp=null), dict(A=null), dict(wfold=null)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*null pointer"):
            tail(**kw)
    for B in (0, -3):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*B=" + str(B)):
            tail(B=B)
    for name, kw in (("x", dict(x=null)), ("score", dict(score=null)), ("emap", dict(emap=null))):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`%s` is NULL" % name):
            tail(**kw)
    for name, kw in (("in", dict(inp=odd)), ("x", dict(x=odd)), ("out", dict(out=odd)), ("emap", dict(emap=odd))):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`%s`.*16-byte aligned" % name):
            tail(**kw)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`emap`.*16-byte aligned"):
        tail(emap=odd, V=14)                               # the pointer is judged before the shape
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-1\).*`emap` is NULL"):
        tail(emap=null, out=null)                          # `out` stays optional, the map does not
    for kw in (dict(T=11), dict(V=14), dict(Ci=8), dict(Co=3)):
        with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\): unsupported layer_tail_map shape"):
            tail(**kw)
    with pytest.raises(_lib.CoskadHipError, match=r"failed \(-2\): unsupported"):
        tail(out=null, Co=3)


def test_ops_wrapper_checks_on_the_host():
    T, V, Ci = 8, 17, 16
    x_in, A, Tm = torch.zeros(2, Ci, T, V), torch.zeros(T, V, V), torch.zeros(V, T, T)
    with pytest.raises(_lib.CoskadHipError, match="CUDA"):
        ops.layer_tail_map(x_in, A, Tm, torch.zeros(2 * Ci, 16), torch.zeros(16), 2, torch.zeros(2, 2, T, V))


# ---- the wrappers' refusals ---------------------------------------------------------------------------------------------------------------

def _lit(cls_name, yaml_name, **over):
    from coskad_amd import lit as L
    cfg = yaml.load(open(os.path.join(ROOT, "config", "synthetic", yaml_name)), Loader=yaml.FullLoader)
    cfg.update(over)
    args, *_ = init_sub_args(Namespace(**cfg))
    return getattr(L, cls_name)(args)


def test_window_error_map_refusals():
    x = torch.zeros(1, 2, 12, 17)
    enc = _lit("LitEncoder", "euclidean_encoder.yaml")
    enc.model.eval()
    with pytest.raises(ValueError, match="window_error_map: LitEncoder has no decoder"):
        enc.window_error_map(x)
    with pytest.raises(ValueError, match="no decoder"):
        attribution.dataset_error_maps(enc, lambda: [[x]], [], "unused")
    for cls, name in (("LitAutoEncoder", "euclidean_autoencoder.yaml"), ("LitVAE", "spherical_vae.yaml")):
        lit = _lit(cls, name)
        lit.model.train()
        with pytest.raises(ValueError, match="window_error_map: train mode"):
            lit.window_error_map(x)
        lit.model.eval()
        with pytest.raises(ValueError, match=r"expected x \[B, 2, 12, 17\]"):
            lit.window_error_map(torch.zeros(1, 2, 8, 17))
        assert not hasattr(lit, "window_latent_attribution") or cls == "LitAutoEncoder"
    ae = _lit("LitAutoEncoder", "euclidean_autoencoder.yaml")
    ae.model.eval()
    ae.score_type = 'hyp'
    with pytest.raises(ValueError, match="'hyp' has no reconstruction term.*window_latent_attribution"):
        ae.window_error_map(x)
    with pytest.raises(ValueError, match="window_latent_attribution"):
        attribution.dataset_error_maps(ae, lambda: [[x]], [], "unused")


def test_unsupported_reason_is_split_and_keeps_its_answers():
    from coskad_amd.models.sts.ae import STSAE
    for cls, name in (("LitAutoEncoder", "euclidean_autoencoder.yaml"), ("LitVAE", "spherical_vae.yaml")):
        lit = _lit(cls, name)
        lit.model.eval()
        assert attribution.unsupported_reason(lit).startswith("autoencoder / VAE wrappers have a decoder")
    enc = _lit("LitEncoder", "euclidean_encoder.yaml")
    enc.model.eval()
    assert attribution.unsupported_reason(enc) is None and attribution.encoder_unsupported_reason(enc.model) is None
    enc.model.train()
    assert attribution.unsupported_reason(enc) == attribution.encoder_unsupported_reason(enc.model)
    assert "train mode" in attribution.encoder_unsupported_reason(enc.model)
    ae = _lit("LitAutoEncoder", "euclidean_autoencoder.yaml")
    ae.model.eval()
    assert attribution.encoder_unsupported_reason(ae.model) is None
    x = torch.zeros(2, 2, 12, 17)
    ae.model.train()
    with pytest.raises(ValueError, match="window_latent_attribution: train mode"):
        ae.window_latent_attribution(x)
    for kw, V, pattern in ((dict(projector='mlp'), 17, "projector 'mlp'"), (dict(), 14, "V = 14"), (dict(), 18, "V = 18"),
                           (dict(dropout=0.1), 17, "dropout")):
        ae.model = STSAE(2, [32, 16, 32], 64, 16, 12, V, 'sts_gcn', kw.get("projector", "linear"), 'euclidean', kw.get("dropout", 0.0))
        ae.model.eval()
        with pytest.raises(ValueError, match=pattern):
            ae.window_latent_attribution(torch.zeros(2, 2, 12, V))
    vae = _lit("LitVAE", "spherical_vae.yaml")
    assert not hasattr(vae, "window_latent_attribution")
    with pytest.raises(ValueError, match="autoencoder wrapper only"):
        attribution.window_latent_attribution(vae, x)
    with pytest.raises(ValueError, match="autoencoder wrapper only"):
        attribution.window_latent_attribution(enc, x)


# ---- the formula of the route without the kernel ------------------------------------------------------------------------------------------------

class _Fixed(torch.nn.Module):
    """STSAE.reconstruction_map's fallback on a stand-in whose forward returns a known (latent, reconstruction)"""
    from coskad_amd.models.sts.ae import STSAE
    reconstruction_map = STSAE.reconstruction_map

    def __init__(self, z, xr):
        super().__init__()
        self.z, self.xr = z, xr

    def _tail_layer(self, t):
        return None

    def forward(self, X):
        return self.z, self.xr


def test_fallback_formula_on_tiny_tensors():
    x = torch.tensor([[[[1., 2.], [3., 4.]], [[0., 0.], [1., -1.]]]])           # [1, 2, 2, 2]
    xr = torch.tensor([[[[2., 2.], [1., 4.]], [[3., 0.], [1., 1.]]]])
    z = torch.zeros(1, 4)
    Z, rec, emap = _Fixed(z, xr).reconstruction_map(x)
    assert Z is z
    # squared differences: channel 0 [[1, 0], [4, 0]], channel 1 [[9, 0], [0, 4]]; C T V = 8
    np.testing.assert_array_equal(emap.numpy(), np.array([[[10., 0.], [4., 4.]]], dtype=np.float32) / 8)
    np.testing.assert_array_equal(rec.numpy(), np.array([18. / 8], dtype=np.float32))
    assert float(emap.sum()) == float(rec[0])
    assert torch.equal(rec, ((xr - x) ** 2).reshape(1, -1).mean(-1))            # reconstruction_scores' expression


# ---- the files --------------------------------------------------------------------------------------------------------------------------------

def test_save_attribution_suffix(tmp_path):
    gts = {(1, 1): np.zeros(4, dtype=np.int64)}
    trans = torch.tensor([0, 1], dtype=torch.int64)
    meta = torch.tensor([[1, 1, 5, 0], [1, 1, 5, 0]], dtype=torch.int64)
    frames = torch.tensor([[1, 2], [1, 2]], dtype=torch.int32)
    attr = torch.tensor([[[1., 2.], [3., 4.]], [[3., 6.], [5., 8.]]])
    plan = eval_utils.ScorePlan(trans, meta, frames, gts, 2, device="cpu")
    maps = eval_utils.attribution_frames(attr, frames, plan)
    eval_utils.save_attribution(str(tmp_path / "a"), maps, plan)
    eval_utils.save_attribution(str(tmp_path / "b"), maps, plan, suffix="error_map")
    assert sorted(os.listdir(tmp_path / "a")) == ["1_1_attribution.npy", "1_1_persons.npy"]      # the default keeps today's names
    assert sorted(os.listdir(tmp_path / "b")) == ["1_1_error_map.npy", "1_1_persons.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "1_1_attribution.npy"), np.load(tmp_path / "b" / "1_1_error_map.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "1_1_error_map.npy")[0],
                                  np.array([[2., 4.], [4., 6.], [np.nan] * 2, [np.nan] * 2], dtype=np.float32))
    with pytest.raises(ValueError, match="persons"):
        eval_utils.save_attribution(str(tmp_path / "c"), maps, plan, suffix="persons")
