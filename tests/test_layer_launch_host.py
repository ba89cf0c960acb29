"""Host side of the layer launchers (stsgcn_bwd.hip / stsgcn_train.hip): what each of the twelve layer entry points refuses, with
which message, and which refusal comes first when several apply.  Every call here fails a check BEFORE the first launch (the
default arguments carry a zero-byte workspace, the last check of all), so the pointers are plain CPU addresses and no GPU is needed."""
import ctypes
import re

import pytest
import torch

from coskad_amd import _lib

BWD = ["coskad_layer_bwd_f32", "coskad_layer_bwd_z_f32", "coskad_layer_bwd_chain_f32", "coskad_layer_bwd_data_f32"]
STATS = ["coskad_layer_train_stats_f32", "coskad_layer_train_stats_z_f32"]
PREFIX = {"coskad_layer_bwd_f32": "layer_bwd", "coskad_layer_bwd_z_f32": "layer_bwd", "coskad_layer_bwd_chain_f32": "layer_bwd_chain",
          "coskad_layer_bwd_data_f32": "layer_bwd_data", "coskad_layer_bwd_stats_f32": "layer_bwd_stats",
          "coskad_layer_gcn_params_f32": "layer_gcn_params", "coskad_layer_train_stats_f32": "layer_train_stats",
          "coskad_layer_train_stats_z_f32": "layer_train_stats", "coskad_layer_train_fold_f32": "layer_train_fold",
          "coskad_layer_train_moments_f32": "layer_train_moments", "coskad_layer_moment_sums_f32": "layer_moment_sums",
          "coskad_layer_train_fold_sums_f32": "layer_train_fold_sums"}
HUGE = 1 << 40      # a workspace size that passes every size check (only used where another check is known to fire)

_DTYPES = {"float32_p": torch.float32, "float64_p": torch.float64, "int32_p": torch.int32, "int64_p": torch.int64,
           "void_p": torch.float32}
_BUFS = {dt: torch.zeros(64, dtype=dt) for dt in set(_DTYPES.values())}
_SCALAR_DEFAULTS = {"B": 4, "Ci": 16, "Co": 16, "T": 12, "V": 17, "rows": 4, "count": 816.0, "stats_in_rows": 4, "below_Ci": 16,
                    "has_residual": 1}


def _params():
    """{entry point: [parameter names]} from the header (the binding keeps the types only)"""
    with open(_lib.HEADER_PATH) as f:
        decls = _lib._declarations(f.read())
    out = {}
    for d in decls:
        m = re.fullmatch(r".*?\b(\w+)\s*\((.*)\)", d)
        if m and m.group(1) in PREFIX:
            out[m.group(1)] = [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(2).split(",")]
    return out


PARAMS = _params()
PROTOS = _lib.prototypes()


def call(name, **over):
    """The entry point with every pointer a small CPU buffer of the right element type, a 16 -> 16 layer at B = 4, (12, 17), the
    optional chain pointers NULL and a ZERO-byte workspace; `over` replaces arguments by name."""
    args = []
    for pname, ctype in zip(PARAMS[name], PROTOS[name][1]):
        if pname in over:
            args.append(over[pname])
        elif ctype.__name__ in _DTYPES:
            optional = pname in ("stats_in", "below_in", "below_Z", "below_in_slope", "below_stats", "stream")
            args.append(None if optional else _BUFS[_DTYPES[ctype.__name__]])
        else:
            args.append(_SCALAR_DEFAULTS.get(pname, 0))
    unknown = set(over) - set(PARAMS[name])
    assert not unknown, (name, unknown)
    _lib.call(name, *args)


def refused(name, match, **over):
    with pytest.raises(_lib.CoskadHipError, match=match):
        call(name, **over)


_ODD = torch.zeros(66, dtype=torch.float32)


def misaligned():
    """an address 4 bytes past an 8-byte boundary (as a raw address: it stands for a float or a double buffer alike)"""
    v = _ODD[1:] if _ODD.data_ptr() % 8 == 0 else _ODD
    assert v.data_ptr() % 8 == 4
    return ctypes.c_void_p(v.data_ptr())


def ws_query(fn, *a):
    return int(getattr(_lib.lib(), fn)(*a))


def test_the_twelve_entries_are_the_header_s():
    assert set(PARAMS) == set(PREFIX) and len(PARAMS) == 12


# ---- the backward entries -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BWD)
def test_bwd_argument_checks(name):
    who = PREFIX[name]
    for required in ["in", "dU", "A", "Tm", "stat", "Wt", "gamma_t", "dWt", "dgamma_t", "dbeta_t", "ws"] + \
            (["dZ"] if name.endswith("data_f32") else ["dA", "dT"]) + (["Z"] if name.endswith("chain_f32") else []):
        refused(name, rf"\(-1\): {who}: null pointer$", **{required: None})
    for grad in ("gamma_r", "dWr", "dgamma_r", "dbeta_r"):
        refused(name, rf"\(-1\): {who}: residual grads missing$", **{grad: None})
    refused(name, rf"\(-1\): {who}: identity residual needs Ci == Co$", Wr=None, Ci=16, Co=32)
    refused(name, rf"\(-1\): {who}: B=0 Ci=16 Co=16$", B=0)
    refused(name, rf"\(-1\): {who}: B=4 Ci=0 Co=16$", Ci=0)
    refused(name, r"\(-2\): unsupported \(n_frames=11, n_joints=17\)", T=11, ws_bytes=HUGE)


@pytest.mark.parametrize("name", BWD + ["coskad_layer_bwd_stats_f32"])
def test_bwd_channel_and_workspace_checks(name):
    """inside the launcher, behind the (T, V) dispatch: channels first, then the workspace -- every entry reports these as layer_bwd"""
    big = {"stats_out_bytes": HUGE} if name.endswith("stats_f32") else {}
    refused(name, r"\(-2\): layer_bwd: channels \(65,16\) > 64 not supported$", Ci=65, ws_bytes=HUGE, **big)
    refused(name, r"\(-2\): layer_bwd: channels \(16,65\) > 64 not supported$", Co=65, ws_bytes=HUGE, **big)
    for (B, Ci, Co, T, V) in [(4, 16, 16, 12, 17), (9, 32, 64, 12, 25), (1, 2, 32, 12, 14)]:
        need = ws_query("coskad_layer_bwd_ws_bytes", B, Ci, Co, T, V)
        assert need > 0
        refused(name, rf"\(-4\): layer_bwd: workspace {need - 1} < {need} bytes$", B=B, Ci=Ci, Co=Co, T=T, V=V, ws_bytes=need - 1, **big)


def test_bwd_chain_buffer_checks():
    name, who = "coskad_layer_bwd_chain_f32", "layer_bwd_chain"
    x = _BUFS[torch.float32]
    refused(name, rf"\(-1\): {who}: stats_in_rows=0$", stats_in=x, stats_in_rows=0)
    refused(name, rf"\(-1\): {who}: stats_in must be 8-byte aligned$", stats_in=misaligned(), stats_in_bytes=HUGE)
    E = 2 * 16 * 16 + 16
    need = (4 * E + 1) // 2 * 2 * 4 + E * 8
    assert ws_query("coskad_layer_bwd_sums_offset", 4, 16, 16) * 4 + E * 8 == need
    refused(name, rf"\(-4\): {who}: stats_in {need - 1} < {need} bytes$", stats_in=x, stats_in_rows=4, stats_in_bytes=need - 1)
    below = dict(below_in=x, below_Z=x, Ci=32, Co=16, below_Ci=2)
    refused(name, rf"\(-1\): {who}: below_stats must be 8-byte aligned$", below_stats=misaligned(), below_stats_bytes=HUGE, **below)
    refused(name, rf"\(-1\): {who}: below_in / below_Z missing$", below_stats=x, below_stats_bytes=HUGE, Ci=32, Co=16, below_Ci=2)
    refused(name, rf"\(-1\): {who}: below_in / below_Z missing$", below_stats=x, below_stats_bytes=HUGE, below_in=x, Ci=32, Co=16, below_Ci=2)
    for (Ci, Co, bCi) in [(16, 16, 16), (32, 16, 16), (32, 64, 2)]:
        assert ws_query("coskad_layer_bwd_below_rows", 4, Ci, Co, bCi, 12, 17) == 0
        refused(name, rf"\(-2\): {who}: \({Ci} -> {Co}\) cannot form the reductions of a layer with {bCi} input channels$",
                below_stats=x, below_stats_bytes=HUGE, below_in=x, below_Z=x, Ci=Ci, Co=Co, below_Ci=bCi)
    assert ws_query("coskad_layer_bwd_below_rows", 4, 32, 16, 2, 12, 25) == 0       # the fused kernel is built for 17 joints
    refused(name, rf"\(-2\): {who}: \(32 -> 16\) cannot form", below_stats=x, below_stats_bytes=HUGE, V=25, **below)
    rows = ws_query("coskad_layer_bwd_below_rows", 4, 32, 16, 2, 12, 17)
    assert rows == 4
    need = ws_query("coskad_layer_bwd_below_floats", 4, 32, 16, 2, 12, 17) * 4
    refused(name, rf"\(-4\): {who}: below_stats {need - 1} < {need} bytes$", below_stats=x, below_stats_bytes=need - 1, **below)


def test_bwd_stats_checks():
    name, who = "coskad_layer_bwd_stats_f32", "layer_bwd_stats"
    for required in ("in", "dU", "A", "Tm", "stats_out", "rows_out", "ws"):
        refused(name, rf"\(-1\): {who}: null pointer$", **{required: None})
    refused(name, rf"\(-1\): {who}: B=0 Ci=16 Co=16$", B=0)
    refused(name, rf"\(-1\): {who}: stats_out must be 8-byte aligned$", stats_out=misaligned(), stats_out_bytes=HUGE)
    need = ws_query("coskad_layer_bwd_stats_floats", 4, 16, 16, 12, 17) * 4
    refused(name, rf"\(-4\): {who}: stats_out {need - 1} bytes too small$", stats_out_bytes=need - 1)
    refused(name, r"\(-2\): unsupported \(n_frames=11, n_joints=17\)", T=11, stats_out_bytes=HUGE, ws_bytes=HUGE)


def test_gcn_params_checks():
    name, who = "coskad_layer_gcn_params_f32", "layer_gcn_params"
    for required in ("in", "dZ", "A", "Tm", "dA", "dT", "ws"):
        refused(name, rf"\(-1\): {who}: null pointer$", **{required: None})
    refused(name, rf"\(-1\): {who}: B=0 Ci=16$", B=0)
    refused(name, rf"\(-1\): {who}: B=4 Ci=65$", Ci=65, ws_bytes=HUGE)
    for V in (17, 25):
        need = ws_query("coskad_layer_gcn_params_ws_bytes", 12, V)
        refused(name, rf"\(-4\): {who}: workspace too small$", V=V, ws_bytes=need - 1)
    refused(name, r"\(-2\): unsupported \(n_frames=11, n_joints=17\)", T=11, ws_bytes=HUGE)


# ---- the forward (statistics) entries -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", STATS + ["coskad_layer_train_fold_f32", "coskad_layer_train_fold_sums_f32"])
def test_train_argument_checks(name):
    who = PREFIX[name]
    first = {"coskad_layer_train_fold_f32": ["partials"], "coskad_layer_train_fold_sums_f32": ["sums"]}.get(name, ["in", "A", "Tm"])
    ws = [] if name.endswith("fold_sums_f32") else ["ws"]
    for required in first + ["Wt", "gamma_t", "beta_t", "wfold", "bias", "stat"] + ws:
        refused(name, rf"\(-1\): {who}: null pointer$", **{required: None})
    for bn in ("gamma_r", "beta_r"):
        refused(name, rf"\(-1\): {who}: residual BN missing$", **{bn: None})
    refused(name, rf"\(-1\): {who}: identity residual needs Ci == Co$", Wr=None, Ci=16, Co=32)


@pytest.mark.parametrize("name", STATS)
def test_train_stats_size_checks(name):
    who = PREFIX[name]
    refused(name, rf"\(-1\): {who}: B=0 Ci=16 Co=16$", B=0)
    refused(name, r"\(-2\): unsupported \(n_frames=11, n_joints=17\)", T=11, ws_bytes=HUGE)
    refused(name, r"\(-2\): train_stats: C_in=65 > 64 not supported$", Ci=65, ws_bytes=HUGE)
    for Ci in (2, 16, 64):
        need = ws_query("coskad_train_stats_ws_bytes", Ci)
        refused(name, rf"\(-4\): train_stats: workspace {need - 1} < {need} bytes$", Ci=Ci, ws_bytes=need - 1)


def test_train_fold_size_checks():
    name, who = "coskad_layer_train_fold_f32", "layer_train_fold"
    refused(name, rf"\(-1\): {who}: B=0 Ci=16 Co=16 rows=4$", B=0)
    refused(name, rf"\(-1\): {who}: B=4 Ci=16 Co=16 rows=0$", rows=0)
    refused(name, rf"\(-1\): {who}: B=4 Ci=65 Co=16 rows=4$", Ci=65, ws_bytes=HUGE)
    # this entry needs the fp64 sums only (the partial rows are the caller's): 2 (Ci^2 + Ci) doubles, rounded up to 256 bytes --
    # less than coskad_train_stats_ws_bytes(Ci), which the header asks for
    need = (2 * (16 * 16 + 16) * 8 + 255) // 256 * 256
    assert need <= ws_query("coskad_train_stats_ws_bytes", 16)
    refused(name, rf"\(-4\): {who}: workspace {need - 1} too small$", ws_bytes=need - 1)


def test_train_fold_sums_size_checks():
    name, who = "coskad_layer_train_fold_sums_f32", "layer_train_fold_sums"
    refused(name, rf"\(-1\): {who}: count=0 Ci=16 Co=16$", count=0.0)
    refused(name, rf"\(-1\): {who}: count=816 Ci=65 Co=16$", Ci=65)
    refused(name, rf"\(-1\): {who}: count=816 Ci=16 Co=0$", Co=0, Wr=_BUFS[torch.float32])


def test_train_moments_checks():
    name, who = "coskad_layer_train_moments_f32", "layer_train_moments"
    for required in ("in", "A", "Tm", "sums", "ws"):
        refused(name, rf"\(-1\): {who}: null pointer$", **{required: None})
    refused(name, rf"\(-1\): {who}: B=0 Ci=16$", B=0)
    refused(name, rf"\(-1\): {who}: sums must be 8-byte aligned$", sums=misaligned(), ws_bytes=HUGE)
    refused(name, r"\(-2\): unsupported \(n_frames=11, n_joints=17\)", T=11, ws_bytes=HUGE)
    refused(name, r"\(-2\): train_stats: C_in=65 > 64 not supported$", Ci=65, ws_bytes=HUGE)
    need = ws_query("coskad_train_stats_ws_bytes", 16)
    refused(name, rf"\(-4\): train_stats: workspace {need - 1} < {need} bytes$", ws_bytes=need - 1)


def test_moment_sums_checks():
    name, who = "coskad_layer_moment_sums_f32", "layer_moment_sums"
    for bad in (dict(partials=None), dict(sums=None), dict(rows=0), dict(Ci=0), dict(Ci=65)):
        refused(name, rf"\(-1\): {who}: bad argument$", **bad)
    refused(name, rf"\(-1\): {who}: sums must be 8-byte aligned$", sums=misaligned())


# ---- which check fires first --------------------------------------------------------------------------------------------------

def test_order_of_the_checks():
    for name in BWD + STATS + ["coskad_layer_bwd_stats_f32", "coskad_layer_gcn_params_f32", "coskad_layer_train_moments_f32"]:
        refused(name, rf"{PREFIX[name]}: null pointer$", **{"in": None}, T=11, Ci=65)            # arguments before the dispatch
        refused(name, rf"{PREFIX[name]}: B=0 ", B=0, T=11)
    for name in BWD + ["coskad_layer_bwd_stats_f32"]:
        refused(name, r"\(-2\): unsupported ", T=11, Ci=65, Co=65, stats_out_bytes=HUGE) if name.endswith("stats_f32") else \
            refused(name, r"\(-2\): unsupported ", T=11, Ci=65, Co=65)                           # the dispatch before the channels
        kw = {"stats_out_bytes": HUGE} if name.endswith("stats_f32") else {}
        refused(name, r"layer_bwd: channels \(65,65\)", Ci=65, Co=65, ws_bytes=0, **kw)          # channels before the workspace
    for name in BWD:
        refused(name, rf"{PREFIX[name]}: residual grads missing$", dWr=None, Ci=16, Co=32, B=0)  # in the order they are written
        refused(name, rf"{PREFIX[name]}: identity residual", Wr=None, Ci=16, Co=32, B=0)
    for name in STATS + ["coskad_layer_train_moments_f32"]:
        refused(name, r"\(-2\): unsupported ", T=11, Ci=65)
        refused(name, r"train_stats: C_in=65", Ci=65, ws_bytes=0)
    x = _BUFS[torch.float32]
    chain = "coskad_layer_bwd_chain_f32"
    refused(chain, r"stats_in_rows=0$", stats_in=misaligned(), stats_in_rows=0)                  # rows, alignment, size; then below_*
    refused(chain, r"stats_in must be 8-byte aligned$", stats_in=misaligned(), stats_in_bytes=0, below_stats=misaligned())
    refused(chain, r"stats_in 0 < ", stats_in=x, stats_in_bytes=0, below_stats=misaligned())
    refused(chain, r"below_stats must be 8-byte aligned$", below_stats=misaligned(), T=11)
    refused(chain, r"B=0 Ci=16 Co=16$", B=0, stats_in=x, stats_in_rows=0)
    refused("coskad_layer_bwd_stats_f32", r"stats_out must be 8-byte aligned$", stats_out=misaligned(), stats_out_bytes=0, T=11)
    refused("coskad_layer_gcn_params_f32", r"workspace too small$", T=11, ws_bytes=0)            # this entry sizes before it dispatches
