"""ctypes binding of libcoskad_hip.so (the C-ABI HIP library, include/coskad_hip.h).

There is NO fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, Tuple

# torch ships its own libamdhip64; it is loaded FIRST so that this library binds to the same HIP runtime
# (two runtimes in one process do not share devices/streams).
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# COSKAD_LIB: another build of the same library (tools/ab_fused.sh: timing-only A/B variants); the shipped path otherwise
LIB_PATH = os.environ.get("COSKAD_LIB") or os.path.join(_HERE, "libcoskad_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "coskad_hip.h")

_lib = None


class CoskadHipError(RuntimeError):
    pass


def _declarations(text: str) -> List[str]:
    """The header's text without comments and preprocessor lines, one string per `;`-terminated declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    return [d for d in (" ".join(d.split()).strip("} ") for d in text.split(";")) if d]


def _pointer(dtype):
    """The type of a pointer parameter.  It takes None (NULL), a tensor (its data_ptr(); where the header names the element type,
    `dtype`, the tensor's must be that one) and whatever c_void_p takes (c_void_p, ctypes arrays, byref(...), ints).
    This conversion runs once per pointer argument of every launch: a closure, no class attributes, no ctypes object built here."""
    as_pointer = ctypes.c_void_p.from_param
    elem = str(dtype)[6:] if dtype is not None else "void"        # "torch.float32" -> "float32"

    def from_param(obj):
        if obj is None:
            return None
        try:
            addr = obj.data_ptr()
        except AttributeError:
            return as_pointer(obj)
        if dtype is not None and obj.dtype is not dtype:
            raise TypeError(f"expected a {elem} tensor, got {str(obj.dtype)[6:]}")
        return as_pointer(addr)
    return type(elem + "_p", (ctypes.c_void_p,), {"from_param": staticmethod(from_param)})


_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
            "float": ctypes.c_float, "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}
_POINTERS = {"float": _pointer(torch.float32), "double": _pointer(torch.float64), "int": _pointer(torch.int32),
             "long long": _pointer(torch.int64), "void": _pointer(None)}
_RETURNS = dict(_SCALARS, **{"const char*": ctypes.c_char_p})


def _ctype(text: str, symbol: str, table=_SCALARS):
    """The ctypes type of one C type of the header; a type outside the tables is an error (never ctypes' defaults)."""
    words = " ".join(text.replace("*", " * ").split()).replace(" *", "*")
    known = table.get(words)
    if known is None and table is _SCALARS and words.endswith("*"):
        target = " ".join(re.sub(r"\bconst\b", " ", words[:-1]).split())
        # pointer to pointer (`const float* const*`): an array of addresses, any element type
        known = _POINTERS["void"] if target.endswith("*") else _POINTERS.get(target)
    if known is None:
        raise CoskadHipError(f"include/coskad_hip.h: {symbol}: no ctypes mapping for the type `{words}`")
    return known


def prototypes(path: str = HEADER_PATH, text: str = None) -> Dict[str, Tuple[type, List[type]]]:
    """{function name: (restype, [argtypes])} of every prototype in include/coskad_hip.h (or of the header text given)."""
    if text is None:
        with open(path) as f:
            text = f.read()
    protos = {}
    for decl in _declarations(text):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", decl)
        if m is None:
            raise CoskadHipError(f"include/coskad_hip.h: cannot parse the declaration `{decl}`")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        args = []
        for prm in ([] if params in ("", "void") else params.split(",")):
            pm = re.fullmatch(r"(.*?)\b\w+", prm.strip())       # `type name`: every parameter of the header is named
            args.append(_ctype(pm.group(1) if pm else prm, name))
        protos[name] = (_ctype(ret, name, _RETURNS), args)
    return protos


def header_symbols(path: str = HEADER_PATH) -> List[str]:
    """Function names declared in include/coskad_hip.h."""
    return list(prototypes(path))


_nargs: Dict[str, int] = {}     # parameter count of every bound entry point (ctypes itself lets surplus arguments through)


def lib() -> ctypes.CDLL:
    """The library, every entry point of the header bound to its prototype (restype and argtypes) once, at load."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CoskadHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C coskad_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
        dll = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in prototypes().items():
            try:
                fn = getattr(dll, name)
            except AttributeError:
                raise CoskadHipError(f"{LIB_PATH} is stale: it lacks `{name}`, which include/coskad_hip.h declares; rebuild it with "
                                     "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C coskad_amd/csrc`") from None
            fn.restype, fn.argtypes = restype, argtypes
            _nargs[name] = len(argtypes)
        _lib = dll
    return _lib


# Optional per-call timing probe (bench.py): PROBE = {"name": <entry point>, "filter": callable or None,
# "events": []}.  When set, matching calls are bracketed by HIP events on torch's current stream (the
# stream every kernel of this library is enqueued on).
PROBE = None


def call(name: str, *args, tag=None) -> None:
    """Call an `int coskad_*(...)` entry point; raise on a non-zero return.  Arguments are plain values -- tensors, None, Python
    numbers -- converted by the entry point's prototype; a wrong count or a value its parameter does not take is a TypeError."""
    fn = getattr(lib(), name)
    if len(args) != _nargs.get(name, len(args)):
        raise TypeError(f"{name} takes {_nargs[name]} arguments, got {len(args)}")
    try:
        if PROBE is not None and PROBE["name"] == name and (PROBE.get("tag") is None or PROBE["tag"] == tag):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            PROBE["events"].append((e0, e1))
        else:
            rc = fn(*args)
    except ctypes.ArgumentError as e:       # "argument <position>: <what from_param said>"
        raise TypeError(f"{name}: {e}") from None
    if rc != 0:
        msg = lib().coskad_last_error().decode(errors="replace")
        raise CoskadHipError(f"{name} failed ({rc}): {msg}")


def ptr(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def i32(x: int) -> ctypes.c_int:
    return ctypes.c_int(int(x))


def f32(x: float) -> ctypes.c_float:
    return ctypes.c_float(float(x))
