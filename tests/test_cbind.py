"""The ctypes bindings of the five C ABIs are read from their headers (isaacgymdyros_amd/cbind.py).  ctypes passes arguments by position and
checks nothing: a C signature that gained a parameter while the binding kept the old list hands a kernel the NEXT argument as its pointer
(the r5m4 memory fault).  The binding and the header now have one source, so these tests hold it against things the
binding's parser did not produce: a dumb regex over the header, the built library, the host compiler's layout of every struct, and
signatures and structs written out here.  No GPU."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

from isaacgymdyros_amd import abi, amp_disc, amp_policy, build, cbind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABIS = [("dyros_walk.h", "dw_", "abi"), ("dyros_ppo.h", "dwp_", "ppo_update"), ("dyros_amp_disc.h", "dwd_", "amp_disc"),
        ("dyros_amp_policy.h", "dwa_", "amp_policy"), ("dyros_stats.h", "dws_", "episode_stats")]
STRUCTS = {"DwdLoss", "DwaLoss"}          # the structs a prototype takes by value


def _c_kinds(args: str):
    """'const float *p, int32_t B, float x, DwdLoss coef, void *stream' -> ['ptr', 'int', 'float', 'struct', 'ptr']"""
    kinds = []
    for a in [x.strip() for x in args.split(",") if x.strip() and x.strip() != "void"]:
        kinds.append("ptr" if "*" in a else ("float" if a.split()[0] == "float" else ("struct" if a.split()[0] in STRUCTS else "int")))
    return kinds


def _kind(t):
    if t is C.c_void_p or t is C.c_char_p or issubclass(t, C._Pointer):
        return "ptr"
    if issubclass(t, C.Structure):
        return "struct"
    return "float" if t is C.c_float else "int"


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build())


@pytest.mark.parametrize("header, prefix, module", ABIS, ids=[a[1].rstrip("_") for a in ABIS])
def test_ctypes_prototypes_match_the_header(header, prefix, module, lib):
    """For every ABI: the names bound are the names the header declares, the built library exports each and reports the header's ABI
    version; and every prototype has the header's argument count with pointer / integer / float / struct in the same places, and a
    c_char_p result exactly where the header says `const char *`."""
    mod = importlib.import_module("isaacgymdyros_amd." + module)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, src)))
    assert names == sorted(prefix + n for n in mod.EXPORTS)
    api = mod.declare(lib)
    assert sorted(api) == sorted(mod.EXPORTS)
    for fn in names:
        assert hasattr(lib, fn), fn
    version = int(re.search(r"#define\s+%sABI_VERSION\s+(\d+)" % prefix.upper(), src).group(1))
    assert api["abi_version"]() == version == mod.K[prefix.upper() + "ABI_VERSION"]
    protos = {m.group(2): (m.group(1), m.group(3))
              for m in re.finditer(r"\b(void|int|int64_t|const char \*)\s*(%s[a-z_0-9]+)\s*\(([^)]*)\)\s*;" % prefix, src)}
    assert sorted(protos) == names
    for name, (ret, args) in protos.items():
        f = api[name[len(prefix):]]
        got = [_kind(t) for t in f.argtypes]
        assert got == _c_kinds(args), (name, got, _c_kinds(args))
        assert (f.restype is C.c_char_p) == (ret == "const char *"), name
        assert (f.restype is None) == (ret == "void"), name
        assert (f.restype is C.c_int64) == (ret == "int64_t"), name
    assert mod.declare(lib) is api          # a library is bound once per process


def test_signatures_written_out():
    """One prototype of every kind the parser maps, with exact ctypes classes: the signature that faulted in round 5, an int64_t by value,
    a struct by value, struct pointers and an out handle, an int64_t result, a string result, no result."""
    P, I, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    from isaacgymdyros_amd import ppo_update
    walk = cbind.signatures("dyros_walk.h", "dw_", abi.STRUCTS)
    dwp = cbind.signatures("dyros_ppo.h", "dwp_", (ppo_update.DwpMlp,))
    dwa = cbind.signatures("dyros_amp_policy.h", "dwa_", (amp_policy.DwaLoss,))
    dwd = cbind.signatures("dyros_amp_disc.h", "dwd_", (amp_disc.DwdLoss,))
    assert (walk, dwp, dwa, dwd) == (cbind.signatures("dyros_walk.h", "dw_"), cbind.signatures("dyros_ppo.h", "dwp_"),      # the default:
                                     cbind.signatures("dyros_amp_policy.h", "dwa_"), cbind.signatures("dyros_amp_disc.h", "dwd_"))  # the header's own
    assert dwp["rollout_post"] == (C.c_int, [P, P, P, P, I, P, P, P, I, I, F, F, P, P, I, P, P, I, P])
    assert dwp["mlp"] == (C.c_int, [C.POINTER(ppo_update.DwpMlp), P])
    assert walk["step"] == (C.c_int, [P, P, P, I64, P])
    assert walk["step_obs"] == (C.c_int, [P, P, P, I64, P, P, P])
    assert walk["create"] == (C.c_int, [C.POINTER(abi.DwConfig), C.POINTER(abi.DwModel), C.POINTER(abi.DwTaskConst), P])
    assert walk["amp_step"] == (C.c_int, [P, C.POINTER(abi.DwAmpConfig), C.POINTER(abi.DwAmpBuffers), P, P, P, P, C.c_int, P, P])
    assert walk["last_error"] == (C.c_char_p, [])
    assert walk["default_config"] == (None, [C.POINTER(abi.DwConfig)])
    assert dwa["grad"] == (C.c_int, [P] * 8 + [I] * 3 + [amp_policy.DwaLoss, P, P, P, I64, P])
    assert dwa["workspace_bytes"] == (I64, [I] * 4)
    assert dwd["grad"] == (C.c_int, [P, P, I, P, I, P, I, I, P, P, P, amp_disc.DwdLoss, P, P, P, I64, P])
    assert "set_dof_properties" not in walk          # (named in a comment of the header only)


@pytest.mark.parametrize("proto", ["int dwx_f(unsigned int n);",               # a scalar that is not one of the fixed-width names
                                   "int dwx_f(Foo coef, void *stream);",        # a struct by value that has no mirror
                                   "int dwx_f(float x[3]);",                    # an array parameter
                                   "int dwx_f(int32_t, void *stream);",         # a parameter without a name
                                   "long dwx_f(void);",                         # a result type
                                   "int dwx_f(int (*cb)(int), void *stream);"])  # not a prototype the header style allows
def test_a_declaration_outside_the_header_style_is_refused(proto):
    with pytest.raises(TypeError, match="dwx_f"):
        cbind.signatures("none.h", "dwx_", (), source="int dwx_abi_version(void);\n" + proto)
    assert list(cbind.signatures("none.h", "dwx_", (), source="int dwx_abi_version(void);\nint64_t dwx_g(const float *const *z, int64_t n);")) \
        == ["abi_version", "g"]


@pytest.mark.parametrize("body", ["unsigned int n;",                         # a base type that is not one of the fixed-width names
                                  "DwxLater s;",                            # ... or a struct the header has not defined by then
                                  "float a[DWX_M];",                        # a dimension that is neither a number nor a define of the header
                                  "int32_t a : 3;",                         # a bit-field
                                  "union { int32_t i; float f; } u;",       # a union
                                  "struct { int32_t i; } s;",               # a nested, anonymous struct definition
                                  "int (*cb)(int);",                        # a function pointer
                                  "float **p;",                             # a pointer to a pointer
                                  "const float *const *z;",
                                  "float *a[2];"])                          # an array of pointers
def test_a_struct_outside_the_header_style_is_refused(body):
    with pytest.raises(TypeError, match="DwxBad"):
        cbind.structs("none.h", "dwx_", source="#define DWX_N 4\ntypedef struct DwxBad {\n    float x[DWX_N];\n    %s\n} DwxBad;" % body)


@pytest.mark.parametrize("source, named", [("typedef struct DwxBad { int32_t a; } DwxOther;", "DwxBad"),     # tag and typedef name differ
                                           ("typedef struct { int32_t a; } DwxBad;", "unnamed"),
                                           ("typedef struct DwxBad { int32_t a; } DwxBad, *DwxPtr;", "DwxBad")])
def test_a_struct_block_that_was_not_read_is_refused(source, named):
    with pytest.raises(TypeError, match="not read as structs: .*" + named):
        cbind.structs("none.h", "dwx_", source="typedef struct DwxGood { int32_t a; } DwxGood;\n" + source)


def test_structs_written_out():
    """One well-formed header with every form the style allows, against ctypes classes written out here: several declarators of one base
    type, a const pointer, every scalar width, a 2-D array with a macro dimension, an embedded array of an earlier struct; the opaque handle
    typedef is no struct."""
    S = cbind.structs("none.h", "dwx_", source="""
        #define DWX_N 4   /* rows */
        typedef struct DwxIn { int32_t a, b; float v[3]; } DwxIn;
        typedef struct DwxHandle DwxHandle;
        typedef struct DwxOut {
            const float *p, *q;      /* [N] each */
            uint8_t *flags; int64_t *ids;
            double  t;
            int16_t m[DWX_N][2];     /* rows of two */
            uint16_t h; uint8_t c;
            DwxIn   inner[DWX_N], last;
            uint64_t seed; int n; int64_t k;
        } DwxOut;
        int dwx_f(const DwxOut *o, DwxIn i);""")
    assert list(S) == ["DwxIn", "DwxOut"] and [s.__name__ for s in S.values()] == list(S) and all(issubclass(s, C.Structure) for s in S.values())
    assert S["DwxIn"]._fields_ == [("a", C.c_int32), ("b", C.c_int32), ("v", C.c_float * 3)]
    assert S["DwxOut"]._fields_ == [("p", C.c_void_p), ("q", C.c_void_p), ("flags", C.c_void_p), ("ids", C.c_void_p), ("t", C.c_double),
                                    ("m", (C.c_int16 * 2) * 4), ("h", C.c_uint16), ("c", C.c_uint8), ("inner", S["DwxIn"] * 4),
                                    ("last", S["DwxIn"]), ("seed", C.c_uint64), ("n", C.c_int), ("k", C.c_int64)]
    assert (C.sizeof(S["DwxIn"]), C.sizeof(S["DwxOut"]), S["DwxOut"].inner.offset, S["DwxOut"].seed.offset) == (20, 184, 60, 160)
    # a pointer field takes what a c_void_p parameter takes: an address, None, a typed pointer
    o, a = S["DwxOut"](), (C.c_float * 2)()
    o.p, o.q, o.flags = C.addressof(a), C.cast(a, C.POINTER(C.c_float)), None
    assert (o.p, o.q, o.flags) == (C.addressof(a), C.addressof(a), None)


@pytest.mark.parametrize("header, prefix, module", ABIS, ids=[a[1].rstrip("_") for a in ABIS])
def test_struct_layouts_match_the_host_compiler(header, prefix, module, tmp_path):
    """For every ABI: a C program that includes the header prints sizeof(S), and offsetof(S, f) and sizeof(S.f) of every field the binding
    has; built by the compiler of the host emulation (tests/emul) and run, its output is the layout of the ctypes classes.  A field the
    binding lacks shows as another sizeof(S), a reordered or mistyped one as another offset or size.  And, by a regex that is not the
    binding's: the identifiers in front of `,` `;` `[` in each struct's body are the class's field names, in order; the modules' classes
    are these."""
    S = cbind.structs(header, prefix)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    assert re.findall(r"typedef\s+struct\s+(\w+)\s*\{", src) == list(S)
    mod = importlib.import_module("isaacgymdyros_amd." + module)
    for name, cls in S.items():
        body = src[src.index("typedef struct %s {" % name):src.index("} %s;" % name)].split("{", 1)[1]
        assert re.findall(r"([A-Za-z_]\w*)\s*[,;\[]", body) == [f for f, _ in cls._fields_], name
        assert getattr(mod, name) is cls
    lines, want = [], []
    for name, cls in S.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        want.append("%s %d" % (name, C.sizeof(cls)))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
            want.append("%s.%s %d %d" % (name, f, getattr(cls, f).offset, getattr(cls, f).size))
    (tmp_path / "layout.cpp").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0;\n}\n'
                                         % (header, "\n".join(lines)))
    exe = str(tmp_path / "layout")
    subprocess.run([os.environ.get("CXX", "g++"), "-I", os.path.join(ROOT, "include"), "-o", exe, str(tmp_path / "layout.cpp")], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines() == want


def test_the_abi_name_lists_are_the_pointer_tables():
    """The three name lists callers fill the pointer tables by are the structs' fields, every one a plain address."""
    for cls, names in ((abi.DwBuffers, abi.BUFFER_NAMES), (abi.DwAmpBuffers, abi.AMP_BUFFER_NAMES), (abi.DwAmpResetDraws, abi.AMP_RESET_DRAW_NAMES)):
        assert [(n, C.c_void_p) for n in names] == cls._fields_ and C.sizeof(cls) == 8 * len(names) > 0


def test_a_library_of_another_abi_version_or_without_a_symbol_is_refused():
    class Fn:
        restype = argtypes = None

        def __call__(self):
            return 999

    class Lib:
        def __init__(self, lacking=()):
            self.lacking = lacking

        def __getattr__(self, name):
            if not name.startswith("dws_") or name in self.lacking:
                raise AttributeError(name)
            return self.__dict__.setdefault(name, Fn())
    with pytest.raises(RuntimeError, match="dyros_stats.h") as e:
        cbind.declare(Lib(), "dyros_stats.h", "dws_")
    assert isinstance(e.value, cbind.DyrosWalkLibraryError)
    with pytest.raises(AttributeError, match="dws_restart"):
        cbind.declare(Lib(("dws_restart",)), "dyros_stats.h", "dws_")
