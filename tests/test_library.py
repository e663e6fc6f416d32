"""The C-ABI shared library loads on a GPU-less host and exports every symbol that
include/m4depth_hip.h declares; argument validation returns hipErrorInvalidValue
without touching a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name="m4depth_hip.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(m4d_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported():
    from m4depth_amd import _lib
    syms = header_symbols()
    assert len(syms) >= 19
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/m4depth_hip.h but not exported"
    assert sorted(_lib.EXPORTED_SYMBOLS) == syms, "ctypes binding and header disagree"
    assert _lib.lib.m4d_abi_version() == _lib.ABI_VERSION == 6
    assert "gfx950" in _lib.build_info()
    # the experiments header: its symbols are exported by an EXPERIMENTS=1 build and ONLY by it, and the binding knows them all
    exp = header_symbols("m4depth_hip_experiments.h")
    assert sorted(_lib.EXPERIMENT_SYMBOLS) == exp and not set(exp) & set(syms)
    assert _lib.has_experiments == ("+experiments" in _lib.build_info())
    for s in exp:
        assert hasattr(raw, s) == _lib.has_experiments, f"{s}: experiments symbol {'missing from' if _lib.has_experiments else 'present in'} this build"
    # process-wide setters: the product header has ONE, the DSCV kernel selector; the profiling hooks (stamp buffers, the DSCV
    # fallback counter) are declared by the experiments header only, and the ablation mask is gone from both
    assert [s for s in syms if "_set_" in s] == ["m4d_dscv_set_variant"]
    assert {"m4d_wino_set_stamps", "m4d_wino6_set_stamps", "m4d_front_set_stamps", "m4d_dscv_set_stamps",
            "m4d_dscv_set_fallback_counter"} <= set(exp)
    assert "m4d_dscv_set_ablation" not in syms + exp


MINI_HEADER = """\
/* mini.h -- every form the binding's parser reads (and a trap: m4d_fake(int x); ) ( ( */
#ifndef MINI_H_
#define MINI_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define M4D_ABI_VERSION 41   /* 41: + m4d_more(int y); 40: the rest */

typedef struct m4d_tagged {
  const float* src;   /* [n] input */
  float* dst;         /* [n] output ) */
  int a, b;
  long long count;
  float gain;
} m4d_tagged;
typedef struct { const void* p; int n; } m4d_anon;

int m4d_version(void);
long long m4d_count(void);
const char* m4d_name(void);
void m4d_set(int flag);
/* spread over three lines */
int m4d_spread(const float* x, const int d[6],
               const void* const* p, unsigned char* m,
               long long rows, float slope, void* stream);
int m4d_structs(const m4d_tagged* levels, const m4d_anon* maps, int n, void* stream);
long long m4d_sized(long long rows, int C);
void m4d_stamps(unsigned long long* buf, const double* pose, int32_t* idx, const uint8_t* lut);

#ifdef __cplusplus
}
#endif
#endif /* MINI_H_ */
"""


def test_parser_reads_every_declaration_form():
    """parse_header on a literal header: multi-line declarations, comments holding declarations and stray parentheses, the
    version macro with its trailing comment, the extern "C" guard, both typedef forms, the four return types, (void), and
    every parameter rule -- exact restype, argtypes, argument names, struct fields and macro value."""
    from m4depth_amd._lib import parse_header
    i, f, ll, vp = ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.c_void_p
    structs, functions, version = parse_header(MINI_HEADER)
    assert version == 41
    assert list(structs) == ["m4d_tagged", "m4d_anon"] and all(issubclass(s, ctypes.Structure) for s in structs.values())
    assert structs["m4d_tagged"]._fields_ == [("src", vp), ("dst", vp), ("a", i), ("b", i), ("count", ll), ("gain", f)]
    assert structs["m4d_anon"]._fields_ == [("p", vp), ("n", i)]
    tagged, anon = ctypes.POINTER(structs["m4d_tagged"]), ctypes.POINTER(structs["m4d_anon"])
    assert functions == {
        "m4d_version": (i, (), ()),
        "m4d_count": (ll, (), ()),
        "m4d_name": (ctypes.c_char_p, (), ()),
        "m4d_set": (None, (i,), ("flag",)),
        "m4d_spread": (i, (vp, vp, vp, vp, ll, f, vp), ("x", "d", "p", "m", "rows", "slope", "stream")),
        "m4d_structs": (i, (tagged, anon, i, vp), ("levels", "maps", "n", "stream")),
        "m4d_sized": (ll, (ll, i), ("rows", "C")),
        "m4d_stamps": (None, (vp, vp, vp, vp), ("buf", "pose", "idx", "lut")),
    }
    assert list(functions) == ["m4d_version", "m4d_count", "m4d_name", "m4d_set", "m4d_spread", "m4d_structs", "m4d_sized",
                               "m4d_stamps"]
    assert parse_header("int m4d_only(void);") == ({}, {"m4d_only": (i, (), ())}, None)


@pytest.mark.parametrize("declaration", [
    "int m4d_x(size_t n);",
    "int m4d_x(double v);",
    "int m4d_x(m4d_s level, void* stream);",                   # a struct by value
    "int m4d_x(const float* x, widget w);",                     # no type the rules know
    "int m4d_x(int);",                                          # no name: `int` is not read as one
    "int m4d_x(int (*callback)(int), void* stream);",           # a function pointer
    "double m4d_x(int n);",                                     # a return type outside the four
    "int m4d_x(int n)",                                         # half a declaration: no terminator before the next one
    "int other_prefix(int n);",
    "typedef struct { double v; } m4d_t;",
    "typedef struct { float *a, *b; } m4d_t;",
    "typedef struct { int a, b[4]; } m4d_t;",
    "typedef struct { int b[4]; } m4d_t;",                      # a field array is stored inline: not the parameter rule
    "typedef struct { float m[9]; int n; } m4d_t;",
    "#define M4D_DECLARE(a) \\",                                # the continuation line below would be read as a declaration
])
def test_parser_refuses_what_it_has_no_rule_for(declaration):
    """Nothing defaults: a declaration outside the rules raises, and the message quotes it."""
    from m4depth_amd._lib import parse_header
    header = "typedef struct { int n; } m4d_s;\nint m4d_before(int a);\n" + declaration + "\nint m4d_after(void* stream);\n"
    with pytest.raises(ValueError) as err:
        parse_header(header)
    assert declaration.rstrip(";") in str(err.value), str(err.value)


def _declaration(txt, name):
    """The comment-stripped text between the parentheses of ``name``'s declaration."""
    (params,) = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    return params


def test_binding_is_the_header():
    """Every function bound on ``lib`` carries exactly the restype and argtypes derived from the headers; the derived
    argument count equals an independent count of the declaration's comma-separated parameters; the parser's names are
    header_symbols()'s."""
    from m4depth_amd import _lib
    for header, table, symbols in (("m4depth_hip.h", _lib.SIGNATURES, _lib.EXPORTED_SYMBOLS),
                                   ("m4depth_hip_experiments.h", _lib.EXPERIMENT_SIGNATURES, _lib.EXPERIMENT_SYMBOLS)):
        assert sorted(table) == sorted(symbols) == header_symbols(header)
        txt = open(os.path.join(ROOT, "include", header)).read()
        for name in symbols:
            restype, argtypes, argnames = table[name]
            params = _declaration(txt, name).strip()
            count = 0 if params in ("", "void") else params.count(",") + 1
            assert len(argtypes) == len(argnames) == count, name
            assert all(re.fullmatch(r"[A-Za-z_]\w*", n) for n in argnames) and len(set(argnames)) == count, (name, argnames)
            if table is _lib.SIGNATURES or _lib.has_experiments:
                fn = getattr(_lib.lib, name)
                assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name
    assert _lib.SIGNATURES["m4d_pyramid_reset"][1][0] is ctypes.POINTER(_lib.ResetLevel)
    assert _lib.SIGNATURES["m4d_normalize_levels"][1][0] is ctypes.POINTER(_lib.NormLevel)
    assert _lib.SIGNATURES["m4d_build_info"][0] is ctypes.c_char_p and _lib.SIGNATURES["m4d_dscv_set_variant"][0] is None
    assert _lib.SIGNATURES["m4d_launch_count"][0] is ctypes.c_longlong
    status = {n: a for n, (r, a, _) in _lib.SIGNATURES.items() if r is ctypes.c_int}
    assert status.pop("m4d_abi_version") == () and _lib._SIGNATURES == status


def test_struct_layout_matches_the_compiler(tmp_path):
    """sizeof and every offsetof of EVERY struct the parser finds in the header, as the host C compiler lays them out, against
    the derived ``ctypes.Structure`` classes."""
    import shutil
    import subprocess
    from m4depth_amd import _lib
    cc = next((p for p in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang", path="/opt/rocm/llvm/bin"),
                           shutil.which("clang", path="/opt/rocm/lib/llvm/bin")) if p), None)
    if cc is None:
        pytest.skip("no host C compiler")
    header = open(os.path.join(ROOT, "include", "m4depth_hip.h")).read()
    classes = _lib.parse_header(header)[0]
    assert sorted(classes) == sorted(re.findall(r"\}\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert classes["m4d_reset_level"]._fields_ == _lib.ResetLevel._fields_
    assert classes["m4d_norm_level"]._fields_ == _lib.NormLevel._fields_
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "m4depth_hip.h"', 'int main(void) {']
    for name, cls in classes.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));' for field, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")],
                   check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiled = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    derived = {}
    for name, cls in classes.items():
        derived[name] = ctypes.sizeof(cls)
        derived.update({f"{name}.{field}": getattr(cls, field).offset for field, _ in cls._fields_})
    assert compiled == derived
    assert derived["m4d_reset_level"] == ctypes.sizeof(_lib.ResetLevel) == 72
    assert derived["m4d_norm_level"] == ctypes.sizeof(_lib.NormLevel) == 32


def test_product_library_exports_only_the_header(tmp_path):
    """Every m4d_* symbol the shared library exports is declared in include/m4depth_hip.h (or, in an experiments build, in
    include/m4depth_hip_experiments.h): no undeclared entry points, no experiment kernels behind global setters in the
    product library."""
    import subprocess
    from m4depth_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("m4d_")})
    allowed = set(header_symbols())
    if _lib.has_experiments:
        allowed |= set(header_symbols("m4depth_hip_experiments.h"))
    extra = [e for e in exported if e not in allowed]
    assert not extra, f"exported but not declared: {extra}"


def test_argument_validation_without_gpu():
    from m4depth_amd._lib import lib
    dims = (ctypes.c_int * 6)(1, 4, 4, 1, 1, 3)
    assert lib.m4d_backproject_fwd(None, None, dims, None, None) == 1
    assert lib.m4d_dense_image_warp(None, None, 1, 4, 4, 1, None, None, None) == 1
    assert lib.m4d_sncv_fwd(None, None, 1, 4, 4, 4, 1, 1, 1, None, 9, None) == 1
    assert lib.m4d_normalize_cuts(None, 1, 4, 4, 4, 1, None, None) == 1
    assert lib.m4d_bias_act(None, None, 4, 4, 0.1, None, None) == 1
    # the staggered first round is a validated per-launch argument (ABI 6), not library state
    assert lib.m4d_conv3x3_wino6_bias_act_ks(None, None, None, 1, 16, 16, 32, 64, 64, 0.1, None, 0, 0, 0, None) == 1
    assert not hasattr(ctypes.CDLL(__import__("m4depth_amd")._lib.LIB_PATH), "m4d_wino6_set_stagger")
    fake = ctypes.c_void_p(4096)           # never dereferenced: validation fails first
    assert lib.m4d_dense_image_warp(fake, fake, 1, 1, 4, 1, fake, None, None) == 1          # H < 2
    assert lib.m4d_sncv_fwd(fake, fake, 1, 4, 4, 6, 1, 1, 4, fake, 36, None) == 1            # cuts do not divide C
    assert lib.m4d_dscv_fwd(fake, fake, fake, fake, fake, 5, fake, fake, fake, 1, 4, 4, 4, 1, 1, 0,
                            fake, 3, None, None, 0, 1.0, None, None) == 1                    # rot_c not in {3,4}


def test_dinl_workspace_covers_double_partials():
    """m4d_dinl_workspace_floats(b, C): the double partial sums of every DINL entry point (512 workgroups x C channels of the
    two-pass forms; 256 workgroups x 32 moments of the single-pass level-0 statistics), then the mean / var tail of 2*b*C floats
    that encoder_head reads at the end; m4d_enc_level0_stats rejects a workspace that is not 8-byte aligned."""
    from m4depth_amd._lib import lib
    for b in (1, 2, 7, 64):
        for C in (16, 32):
            n = lib.m4d_dinl_workspace_floats(b, C)
            assert n >= b * 512 * C * 2 + 2 * b * C, (b, C, n)
        assert lib.m4d_dinl_workspace_floats(b, 16) >= b * 256 * 32 * 2 + 2 * b * 16
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)      # never dereferenced: validation fails first
    assert lib.m4d_enc_level0_stats(fake, 1, 0, 0, fake, fake, 1, 4, 4, odd, fake, fake, None) == 1


def test_missing_library_is_loud(monkeypatch, tmp_path):
    import importlib
    from m4depth_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU / PyTorch fallback"):
        _lib._load()


def test_cpu_tensor_is_rejected():
    import torch
    import m4depth_amd as M
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.dense_image_warp(torch.zeros(1, 4, 4, 1), torch.zeros(1, 4, 4, 2))


def test_launch_tape_bookkeeping_without_gpu():
    """m4d_tape_begin / _end / _length / _free (csrc/m4d_tape.hip): an empty recording is a valid tape of length 0, nested
    recordings are refused, unknown ids are errors -- no device involved."""
    from m4depth_amd import _lib
    from m4depth_amd._lib import lib
    if not _lib.has_experiments:
        pytest.skip("the launch tape is an experiment: make EXPERIMENTS=1 (include/m4depth_hip_experiments.h)")
    t = lib.m4d_tape_begin()
    assert t >= 0
    assert lib.m4d_tape_begin() == -1                       # this thread is already recording
    assert lib.m4d_tape_replay(t, None) != 0                # a tape cannot be replayed while it records
    assert lib.m4d_tape_end() == 0 and lib.m4d_tape_end() == -1
    assert lib.m4d_tape_length(t) == 0 and lib.m4d_tape_length(t + 1000) == -1
    assert lib.m4d_tape_free(t) == 0 and lib.m4d_tape_free(t) != 0 and lib.m4d_tape_length(t) == -1


def test_integration_doc_lists_exactly_the_switches_the_package_reads():
    """INTEGRATION.md section 4 has one table row per ``M4D_*`` environment variable named in m4depth_amd/*.py, and no other:
    a switch cannot be added, or retired, without the document following."""
    import glob
    in_code = set()
    for path in glob.glob(os.path.join(ROOT, "m4depth_amd", "*.py")):
        in_code |= set(re.findall(r"\bM4D_[A-Z0-9_]+", open(path).read()))
    in_code.discard("M4D_ABI_VERSION")                   # the header's version macro (named in a comment of _lib.py), no switch
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    in_table = _doc_table_switches("## 4. Kernel-selection switches")
    assert in_table == in_code, (sorted(in_code - in_table), sorted(in_table - in_code))


def _doc_table_switches(heading):
    """The ``M4D_*`` names in the first column of the table under INTEGRATION.md's section ``heading`` (up to the next ``## ``)."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index(heading) + len(heading):]
    section = section[:section.index("\n## ")] if "\n## " in section else section
    names = set()
    for line in section.splitlines():
        if line.startswith("| `M4D_"):
            names |= set(re.findall(r"\bM4D_[A-Z0-9_]+", line.split("|")[1]))
    return names


LIBRARY_SWITCH_DEFAULTS = {"sncv_variant": 1, "sncv_ys": 0, "sncv_small_px": 6000, "wino_variant": 4, "wino4_min_wg": 100,
                           "dscv_bwd_window_kb": 48}


def test_library_reads_the_environment_only_in_its_switch_table():
    """Comments stripped, ``getenv`` occurs under m4depth_amd/csrc and tools/experiments/csrc only in the translation unit that
    defines m4d_switches(), and the ``M4D_*`` names read there are the rows of INTEGRATION.md section 5, no more and no fewer."""
    readers, names = [], set()
    for d in (os.path.join(ROOT, "m4depth_amd", "csrc"), os.path.join(ROOT, "tools", "experiments", "csrc")):
        for n in sorted(os.listdir(d)):
            if not n.endswith((".hip", ".h", ".hpp", ".cpp")):
                continue
            code = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(d, n)).read(), flags=re.S)
            if re.search(r"\bgetenv\b", code):
                readers.append(n)
                assert re.search(r"\bm4d_switches\s*\(\s*\)\s*\{", code), f"{n} reads the environment but does not define m4d_switches()"
                names |= set(re.findall(r'"(M4D_[A-Z0-9_]+)"', code))
    assert readers == ["m4d_api.hip"], readers
    assert names == _doc_table_switches("## 5. Switches of the library itself")
    assert {n[4:].lower() for n in names} == set(LIBRARY_SWITCH_DEFAULTS)


def _child(call, restype, **env):
    """``call`` on the library in a fresh process (plain ctypes: no package import, a fraction of a second) with the M4D_*
    variables of ``env`` and no others."""
    import subprocess, sys
    from m4depth_amd import _lib
    full = {k: v for k, v in os.environ.items() if not k.startswith("M4D_")}
    full.update(env)
    code = (f"import ctypes; f = ctypes.CDLL({_lib.LIB_PATH!r}).{call}; f.restype = ctypes.{restype}; r = f(); "
            "print(r.decode() if isinstance(r, bytes) else r)")
    r = subprocess.run([sys.executable, "-c", code], env=full, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip()


def test_switches_info_reflects_the_environment():
    """m4d_switches_info() in a child process: the defaults of INTEGRATION.md section 5 with nothing set, the environment's values
    with every kept variable set to something else (M4D_DSCV_BWD_WINDOW_KB clamped to 0..64)."""
    show = ("m4d_switches_info", "c_char_p")
    parse = lambda text: {k: int(v) for k, v in (item.split("=") for item in text.split())}
    assert parse(_child(*show)) == LIBRARY_SWITCH_DEFAULTS
    other = {"sncv_variant": 0, "sncv_ys": 2, "sncv_small_px": 100000, "wino_variant": 2, "wino4_min_wg": 7, "dscv_bwd_window_kb": 16}
    assert parse(_child(*show, **{"M4D_" + k.upper(): str(v) for k, v in other.items()})) == other
    assert parse(_child(*show, M4D_DSCV_BWD_WINDOW_KB="200"))["dscv_bwd_window_kb"] == 64
    assert parse(_child(*show, M4D_DSCV_BWD_WINDOW_KB="-3"))["dscv_bwd_window_kb"] == 0


def test_a_retired_switch_is_not_read():
    """M4D_WINO6P_MIN_UNITS moved the persistent-kernel threshold until it was retired: the library answers 2048 whatever it says."""
    assert _child("m4d_wino6_persistent_min_units", "c_longlong", M4D_WINO6P_MIN_UNITS="900") == "2048"


def test_library_sources_enqueue_no_memset():
    """Every zero-fill of the library is a kernel launch (m4d_zero_f32, csrc/m4d_common.h).  A hipMemsetAsync captured into the
    training graph becomes a memset node, and those were not reliably ordered against the kernel nodes around them on replay:
    the scatter backwards summed onto stale or half-cleared buffers in some replays."""
    src = os.path.join(ROOT, "m4depth_amd", "csrc")
    names = [n for n in sorted(os.listdir(src)) if n.endswith((".hip", ".h", ".cpp"))]
    assert "m4d_grad.hip" in names and "m4d_warp.hip" in names
    for n in names:
        code = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(src, n)).read(), flags=re.S)
        assert not re.search(r"\bhipMemset\w*\s*\(", code), f"csrc/{n} enqueues a memset"
