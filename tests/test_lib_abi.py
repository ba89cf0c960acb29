"""CPU-side checks of the C-ABI library: it loads, exports every symbol the header declares, every entry point is bound to the
header's prototype, and its argument validation fails loudly (no kernel is launched here)."""
import ast
import ctypes
import os

import pytest

from coskad_amd import _lib


def test_library_built_and_loads():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = _lib.lib()
    assert lib.coskad_abi_version() == 1


def test_every_header_symbol_is_exported():
    lib = _lib.lib()
    syms = _lib.header_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_exported_symbols_are_declared():
    """no stray extern "C" entry point without a header declaration"""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("coskad_")}
    assert exported == set(_lib.header_symbols())


def test_argument_errors_are_reported_without_a_gpu():
    null = ctypes.c_void_p(0)
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        _lib.call("coskad_gcn_f32", null, null, null, null, _lib.i32(4), _lib.i32(12), _lib.i32(17), _lib.i32(0), null)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    with pytest.raises(_lib.CoskadHipError, match="unsupported"):
        _lib.call("coskad_gcn_f32", p, p, p, p, _lib.i32(4), _lib.i32(11), _lib.i32(17), _lib.i32(0), null)
    with pytest.raises(_lib.CoskadHipError, match="latent"):
        _lib.call("coskad_btlnk_fwd_f32", p, p, p, null, p, _lib.i32(4), _lib.i32(816), _lib.i32(64), null)


def test_prototypes_cover_the_header():
    """every declaration of the header parses into (restype, argtypes); nothing is left to ctypes' defaults"""
    protos = _lib.prototypes()
    assert list(protos) == _lib.header_symbols() and len(protos) == len(set(_lib.header_symbols()))
    assert len(protos["coskad_gcn_f32"][1]) == 9
    assert protos["coskad_train_stats_ws_bytes"][0] is ctypes.c_size_t
    gemm = protos["coskad_gemm_f32"][1]
    assert [i for i, t in enumerate(gemm) if t is ctypes.c_longlong] == list(range(4, 13)) + [22]
    assert protos["coskad_bn2_apply_prelu_f32"][1][-2:] == [ctypes.c_float, ctypes.c_ulonglong]
    assert protos["coskad_last_error"] == (ctypes.c_char_p, [])
    lib = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


@pytest.mark.parametrize("decl, word", [("int coskad_x(short n);", "short"), ("long coskad_x(int n);", "long"),
                                        ("int coskad_x(const char* s);", "char"), ("int coskad_x(unsigned n);", "unsigned")])
def test_an_unknown_type_in_the_header_is_an_error(decl, word, tmp_path):
    with pytest.raises(_lib.CoskadHipError, match=rf"coskad_x.*{word}"):
        _lib.prototypes(text="/* a header */\n#include <x.h>\nint coskad_ok(const float* p, size_t n);\n" + decl)
    path = tmp_path / "h.h"
    path.write_text(decl)
    with pytest.raises(_lib.CoskadHipError, match=rf"coskad_x.*{word}"):
        _lib.prototypes(str(path))


# call sites that build their argument list (`*args`): the count is not visible to the syntax tree, only the name is checked
STARRED_CALLS = {"coskad_layer_train_stats_f32", "coskad_layer_train_stats_z_f32", "coskad_layer_bwd_chain_f32", "coskad_layer_bwd_f32",
                 "coskad_layer_bwd_z_f32", "coskad_lowrank_fold_fwd_f32"}


def test_every_call_site_in_ops_matches_its_prototype():
    from coskad_amd import ops
    protos = _lib.prototypes()
    with open(ops.__file__) as f:
        tree = ast.parse(f.read())
    counted, starred, attrs = 0, set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and node.attr.startswith("coskad_"):
            attrs.add(node.attr)
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "call"):
            continue
        name = node.args[0]
        assert isinstance(name, ast.Constant) and isinstance(name.value, str), f"line {node.lineno}: entry point is not a literal"
        assert name.value in protos, name.value
        assert [k.arg for k in node.keywords] in ([], ["tag"]), f"line {node.lineno}"
        if any(isinstance(a, ast.Starred) for a in node.args):
            starred.add(name.value)
        else:
            assert len(node.args) - 1 == len(protos[name.value][1]), f"line {node.lineno}: {name.value}"
            counted += 1
    assert starred == STARRED_CALLS
    assert counted >= 60
    assert attrs and attrs <= set(protos), attrs - set(protos)       # the `_lib.lib().coskad_*` size / support queries


def test_the_boundary_rejects_mistyped_arguments():
    """what the untyped binding let through: a wrong count, a float for an int, a tensor of another element type"""
    import torch
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = (p, p, p, p, 4, 11, 17, 0, None)                 # T = 11: refused ("unsupported") before the device is touched
    with pytest.raises(_lib.CoskadHipError, match="unsupported"):
        _lib.call("coskad_gcn_f32", *good)
    with pytest.raises(TypeError, match="coskad_gcn_f32 takes 9 arguments, got 8"):
        _lib.call("coskad_gcn_f32", *good[:-1])
    with pytest.raises(TypeError, match="coskad_gcn_f32 takes 9 arguments, got 10"):
        _lib.call("coskad_gcn_f32", *good, None)
    with pytest.raises(TypeError, match="coskad_gcn_f32: argument 5"):
        _lib.call("coskad_gcn_f32", p, p, p, p, 4.0, 11, 17, 0, None)
    x = torch.zeros(16)
    with pytest.raises(_lib.CoskadHipError, match="unsupported"):       # a CPU tensor is only an address here; float32 passes
        _lib.call("coskad_gcn_f32", x, x, x, x, 4, 11, 17, 0, None)
    with pytest.raises(TypeError, match=r"coskad_gcn_f32: argument 1: .*float32.*int64"):
        _lib.call("coskad_gcn_f32", torch.zeros(16, dtype=torch.int64), x, x, x, 4, 11, 17, 0, None)
    with pytest.raises(_lib.CoskadHipError, match="null pointer"):
        _lib.call("coskad_gcn_f32", None, None, None, None, 4, 12, 17, 0, None)
    with pytest.raises(_lib.CoskadHipError, match="latent"):
        _lib.call("coskad_btlnk_fwd_f32", x, x, x, None, x, 4, 816, 64, None)
    with pytest.raises(ctypes.ArgumentError):                           # the size queries are bound as well
        _lib.lib().coskad_stat_floats(32.0, 64)


def test_size_queries():
    lib = _lib.lib()
    lib.coskad_stat_floats.restype = ctypes.c_int
    assert lib.coskad_stat_floats(32, 64) == 2 * 32 + 2 * 64 * 32 + 4 * 64
    lib.coskad_head_slots.restype = ctypes.c_int
    assert lib.coskad_head_slots() == 19
    lib.coskad_train_stats_ws_bytes.restype = ctypes.c_size_t
    assert lib.coskad_train_stats_ws_bytes(32) > 512 * 2 * (32 * 32 + 32) * 4


def test_python_layer_fits_agrees_with_the_library():
    """`ST_GCNN_layer.is_wide` decides in Python (no native call while a model is built); same answer as coskad_layer_fits."""
    from coskad_amd import ops
    from coskad_amd.models.graph_layers.stsgcn import layer_fits
    for V in (14, 17, 18, 25):
        for Ci in (1, 2, 3, 4, 8, 16, 32, 48, 64, 65, 128):
            for Co in (2, 16, 32, 64, 65, 256):
                assert layer_fits(Ci, Co, 12, V) == ops.layer_fits(Ci, Co, 12, V), (Ci, Co, V)
