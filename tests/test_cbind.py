"""The ctypes bindings of the five C ABIs are read from their headers (isaacgymdyros_amd/cbind.py).  ctypes passes arguments by position and
checks nothing: a C signature that gained a parameter while the binding kept the old list hands a kernel the NEXT argument as its pointer
(the r5m4 memory fault).  The binding and the header now have one source, so these tests hold it against things the
binding's parser did not produce: a dumb regex over the header, the built library, and signatures written out here.  No GPU."""
import ctypes as C
import importlib
import os
import re

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
