"""ctypes binding to libm4depth_hip.so (the C ABI of include/m4depth_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call
returns a HIP error, this raises.  PyTorch is used only as the owner of device
memory and streams (``tensor.data_ptr()``, ``torch.cuda.current_stream()``).
"""
from __future__ import annotations

import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# M4D_LIB_FLAVOUR=experiments selects the `make EXPERIMENTS=1` library (libm4depth_hip_exp.so: the product kernels + the
# measured-and-not-dispatched ones of tools/experiments/csrc with their process-global selectors); anything else = the product
LIB_FLAVOUR = os.environ.get("M4D_LIB_FLAVOUR", "product")
LIB_PATH = os.path.join(_HERE, "libm4depth_hip_exp.so" if LIB_FLAVOUR == "experiments" else "libm4depth_hip.so")

_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
_RESTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "void": None, "const char*": ctypes.c_char_p}
_TYPEDEF = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(m4d_\w+)\s*\(([^()]*)\)")
_DECLARATOR = re.compile(r"([\w\s*]*?)(\w+)\s*(\[\d*\])?")


def parse_header(text):
    """The C ABI of a header as ctypes: ``(structs, functions, abi_version)``.

    structs: typedef name -> ``ctypes.Structure`` class; functions: ``m4d_*`` name -> (restype, argtypes, argnames), in the
    header's order; abi_version: the value of ``M4D_ABI_VERSION`` (None when the header defines none).  The rules, all of them:
      - scalars: ``int`` -> c_int, ``float`` -> c_float, ``long long`` -> c_longlong; ``const`` is ignored;
      - return types: ``int``, ``long long``, ``void`` (None) and ``const char*`` (c_char_p);
      - a parameter that points to a struct typedef'd anywhere in the same header -> POINTER(that Structure); a struct field
        sees only the structs typedef'd before its own;
      - every other pointer or array parameter (``const float* x``, ``const int dims[6]``, ``const void* const* maps``,
        ``void* stream``, ...) -> c_void_p: the header cannot tell a host array from a device pointer;
      - struct fields follow the scalar and pointer rules; ``int a, b;`` declares several scalars; both ``typedef struct tag
        {...} name;`` and ``typedef struct {...} name;`` are read;
      - anything else (another scalar type, a struct by value, a function pointer, an array as a struct FIELD -- it is stored
        inline, not as a pointer --, a preprocessor line continued with a backslash, text that is no declaration) raises
        ValueError quoting the declaration.  Nothing defaults."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    continued = re.search(r"^[ \t]*#.*\\[ \t]*$", text, re.M)
    if continued:
        raise ValueError(f"m4depth_amd: no rule for a continued preprocessor line, `{continued.group(0).strip()}`")
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+M4D_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, re.M)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                                  # guards, includes, the macro
    text = re.sub(r'extern\s+"C"\s*\{|^[ \t]*\}[ \t]*$', "", text, flags=re.M)           # ... and what they wrap
    structs = {}

    def ctype(decl, where):
        """(ctypes type, name) of one ``type name`` / ``type name[n]`` declarator."""
        m = _DECLARATOR.fullmatch(decl.strip())
        base = " ".join(w for w in (m.group(1).replace("*", " ") if m else "").split() if w != "const")
        if m and base and (m.group(3) or "*" in m.group(1)):
            struct = structs.get(base) if m.group(1).count("*") == 1 and not m.group(3) else None
            return (ctypes.POINTER(struct) if struct else ctypes.c_void_p), m.group(2)
        if base not in _SCALARS:
            raise ValueError(f"m4depth_amd: no ctypes rule for `{decl.strip()}` in `{' '.join(where.split())}`")
        return _SCALARS[base], m.group(2)

    def typedef(m):
        fields = []
        for line in filter(None, (f.strip() for f in m.group(1).split(";"))):
            first, *more = (d.strip() for d in line.split(","))
            t, name = ctype(first, m.group(0))
            if "[" in line or more and (t not in _SCALARS.values() or not all(re.fullmatch(r"\w+", d) for d in more)):
                raise ValueError(f"m4depth_amd: no rule for an array field, and only plain scalars share a line: `{line}` of "
                                 f"`{' '.join(m.group(0).split())}`")
            fields += [(name, t)] + [(d, t) for d in more]
        structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
        return ""

    functions = {}
    for stmt in filter(None, (s.strip() for s in _TYPEDEF.sub(typedef, text).split(";"))):
        m = _FUNCTION.fullmatch(stmt)
        ret = re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())) if m else None
        if ret not in _RESTYPES:
            raise ValueError(f"m4depth_amd: no ctypes rule for the declaration `{' '.join(stmt.split())}`")
        params = [] if m.group(3).strip() in ("", "void") else [ctype(p, stmt) for p in m.group(3).split(",")]
        functions[m.group(2)] = (_RESTYPES[ret], tuple(t for t, _ in params), tuple(n for _, n in params))
    return structs, functions, int(version.group(1)) if version else None


def _parse(name):
    with open(os.path.join(_INCLUDE, name)) as f:
        return parse_header(f.read())


# include/m4depth_hip.h is the only statement of the ABI: the signatures, both structs and the version are read from it
_structs, SIGNATURES, ABI_VERSION = _parse("m4depth_hip.h")                     # ABI_VERSION = the header's M4D_ABI_VERSION
NormLevel, ResetLevel = _structs["m4d_norm_level"], _structs["m4d_reset_level"]
# include/m4depth_hip_experiments.h: present only in a `make EXPERIMENTS=1` build of the library (the launch tape and the
# selectors of the not-dispatched Winograd kernels); bound when the library has them, ``has_experiments`` says whether
EXPERIMENT_SIGNATURES = _parse("m4depth_hip_experiments.h")[1]
EXPORTED_SYMBOLS, EXPERIMENT_SYMBOLS = list(SIGNATURES), list(EXPERIMENT_SIGNATURES)
# the entry points that return a HIP status (launches and `_supported` queries) -> argtypes: what the launch recorder of
# tests/test_level_dispatch.py wraps; a view of SIGNATURES, nothing is stated here
_SIGNATURES = {n: a for n, (r, a, _) in SIGNATURES.items() if r is ctypes.c_int and n != "m4d_abi_version"}


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"m4depth_amd: native library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C m4depth_amd/csrc`. "
            "There is no CPU / PyTorch fallback for the hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    for table in (SIGNATURES, EXPERIMENT_SIGNATURES if hasattr(lib, "m4d_tape_begin") else {}):
        for name, (restype, argtypes, _) in table.items():
            fn = getattr(lib, name)          # AttributeError if the .so is stale: loud by design
            fn.restype = restype
            fn.argtypes = argtypes
    if lib.m4d_abi_version() != ABI_VERSION:     # the library was built from another header
        raise ImportError(f"m4depth_amd: ABI mismatch, library reports {lib.m4d_abi_version()}, binding expects {ABI_VERSION}")
    return lib


lib = _load()
has_experiments = hasattr(lib, "m4d_tape_begin")      # a `make EXPERIMENTS=1` build (include/m4depth_hip_experiments.h)


def require_experiments(what):
    if not has_experiments:
        raise RuntimeError(f"{what} needs the experiments build of the library: make -C m4depth_amd/csrc EXPERIMENTS=1 "
                           "(-> libm4depth_hip_exp.so, sources in tools/experiments/csrc) and M4D_LIB_FLAVOUR=experiments in "
                           "the environment; the product library exports only the kernels it dispatches")


def build_info() -> str:
    return lib.m4d_build_info().decode()


def switches() -> dict:
    """The environment switches of the library as this process read them (m4d_switches_info): {"sncv_variant": 1, ...}."""
    return {k: int(v) for k, v in (item.split("=") for item in lib.m4d_switches_info().decode().split())}


def assert_switches_follow_env(*variables):
    """Every named variable that the environment sets is the value the library runs with: a comparison between processes that
    differ only in a switch compares nothing if the library ignores it."""
    got = switches()
    for var in variables:
        if var in os.environ:
            assert got[var[4:].lower()] == int(os.environ[var]), f"{var}={os.environ[var]} but the library runs with {got}"


def stream_ptr():
    """The current PyTorch HIP stream as a void* for the C ABI."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t, name="tensor", dtype=torch.float32):
    """Device pointer of a dense CUDA(ROCm) tensor; None -> NULL."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: m4depth_amd ops run on the MI355X only (tensor is on {t.device}); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a dense row-major (NHWC) tensor, got strides {t.stride()}")
    return ctypes.c_void_p(t.data_ptr())


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"m4depth_amd: {what} failed with HIP error {rc}"
                           + (" (hipErrorInvalidValue: bad argument)" if rc == 1 else ""))


# Framework copies inside a hipGraph capture: refused on the inference path (every node of its graph is a library kernel), allowed
# inside ``framework_copies_in_capture()`` -- the TRAINING step's capture, whose autograd graph is made of framework nodes anyway
# (slice copies, gradient accumulation) around the library's kernels.
_capture_copies_ok = [False]


class framework_copies_in_capture:
    def __enter__(self):
        self._old = _capture_copies_ok[0]
        _capture_copies_ok[0] = True
        return self

    def __exit__(self, *exc):
        _capture_copies_ok[0] = self._old
        return False


def as_f32(t, name):
    """Dense float32 device tensor (copies only when a conversion is needed)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    if t.is_cuda and not _capture_copies_ok[0] and torch.cuda.is_current_stream_capturing():
        # a conversion here would put a framework copy kernel into the captured graph (round 4: ~43 per batch-32 step, the
        # [:, t] slices of batch-major rot / trans): the capturing callers hand over dense frame-major tensors instead
        raise RuntimeError(f"{name}: a non-contiguous / non-float32 tensor (shape {tuple(t.shape)}, strides {t.stride()}, "
                           f"{t.dtype}) reached a kernel wrapper inside a hipGraph capture; it would be copied by a framework "
                           "kernel inside the graph -- make it dense before capturing")
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()
