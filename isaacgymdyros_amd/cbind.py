"""ctypes bindings read from the C headers under include/: the header is the one statement of an ABI, and nothing here is kept by hand.

ctypes passes arguments by position and checks nothing, so a prototype that gained a parameter while a hand-written argtypes list kept the
old one hands a kernel the NEXT argument as its pointer.  Hence: The same holds for a struct: a field added in the header while a hand-written mirror kept the old list
shifts every later field.  Hence: `constants()` reads a header's integer #defines, `structs()` turns every `typedef struct X { ... } X;`
into a ctypes.Structure, `signatures()` turns every prototype `ret prefix_name(args);` into ctypes classes, `declare()` sets them on a
loaded library and compares the library's ABI version with the header's.  The headers are written in a narrow style (one declaration per
parameter, every parameter named, fixed-width scalars; struct fields of one base type per declaration, `*name` or `name[DIM][DIM]`); a
declaration outside that style raises, it is never guessed.
"""
from __future__ import annotations

import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
           "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16}


class DyrosWalkLibraryError(RuntimeError):
    pass


def _source(header: str) -> str:
    with open(os.path.join(INCLUDE, header)) as f:
        return f.read()


def constants(header: str, prefix: str, source: str = None) -> dict:
    """Every integer `#define PREFIX_NAME value` of the header (decimal, negative, 0x); defines with another kind of value are left out."""
    return {k: int(v, 0) for k, v in re.findall(r"^[ \t]*#define[ \t]+(%s[A-Z0-9_]+)[ \t]+(-?(?:0x[0-9a-fA-F]+|\d+))(?=\s|$)" % prefix.upper(),
                                                _source(header) if source is None else source, re.M)}


def _field(base: str, text: str, structs: dict, dims: dict):
    """(name, ctypes class) of one declarator of a struct field: `name`, `*name` (any pointer is a plain address, as in _ctype) or
    `name[DIM][DIM]`, DIM a number or one of dims."""
    m = re.fullmatch(r"(\*?)\s*([A-Za-z_]\w*)\s*((?:\[\s*\w+\s*\]\s*)*)", text.strip())
    shape = re.findall(r"\w+", m.group(3)) if m else []
    if m and all(d.isdigit() or d in dims for d in shape):
        t = (None if shape else C.c_void_p) if m.group(1) else SCALARS.get(base) or structs.get(base)
        if t is not None:
            for d in reversed(shape):
                t = t * (int(d) if d.isdigit() else dims[d])
            return m.group(2), t
    raise TypeError("no ctypes class for the field %r" % " ".join((base + " " + text).split()))


class Struct(C.Structure):
    """A pointer field takes what a c_void_p parameter takes: an address, None, or a typed ctypes pointer (stored as its address)."""

    def __setattr__(self, name, value):
        super().__setattr__(name, C.cast(value, C.c_void_p) if isinstance(value, C._Pointer) else value)


_structs = {}


def structs(header: str, prefix: str, source: str = None) -> dict:
    """struct name -> ctypes.Structure class of every `typedef struct X { ... } X;` of the header, in its order, built once per header.
    A declaration is one base type (a name of SCALARS or an earlier struct of the header, `const` ignored) and its declarators, separated
    by commas; array dimensions are numbers or integer #defines of the header.  source: the header's text (tests)."""
    if source is None and header in _structs:
        return _structs[header]
    src = re.sub(r"/\*.*?\*/", " ", _source(header) if source is None else source, flags=re.S)
    dims, out = constants(header, prefix, src), {}
    for struct, body in re.findall(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", src):
        fields = []
        try:
            for decl in filter(None, map(str.strip, body.split(";"))):
                base, rest = (re.sub(r"^const\s+", "", decl).split(None, 1) + [""])[:2]
                fields += [_field(base, text, out, dims) for text in rest.split(",")]
        except TypeError as e:
            raise TypeError("include/%s: %s: %s" % (header, struct, e)) from None
        out[struct] = type(struct, (Struct,), {"_fields_": fields})
    opened = re.findall(r"\btypedef\s+struct\b\s*(\w*)\s*\{", src)
    if opened != list(out):
        raise TypeError("include/%s: not read as structs: %s" % (header, ", ".join(n or "(unnamed)" for n in opened if n not in out)))
    if source is None:
        _structs[header] = out
    return out


def _ctype(text: str, structs: dict, named: bool):
    """The ctypes class of one parameter (named) or return type.  Data pointers stay untyped: the double-precision oracle is bound through
    the float header, and callers hand over plain addresses, ctypes arrays or byref()."""
    words = [w for w in re.findall(r"\w+|\S", text) if w != "const"]
    base, stars = (words[0] if words else ""), (words[1:-1] if named else words[1:])
    if len(words) >= 1 + named and re.fullmatch(r"[A-Za-z_]\w*", base) and all(s == "*" for s in stars):
        if stars:
            if base == "char" and not named:
                return C.c_char_p
            return C.POINTER(structs[base]) if base in structs and len(stars) == 1 else C.c_void_p
        if base in structs:
            return structs[base]
        if base in SCALARS:
            return SCALARS[base]
        if base == "void" and not named:
            return None
    raise TypeError("no ctypes class for %r" % text.strip())


_signatures = {}


def signatures(header: str, prefix: str, classes=None, source: str = None) -> dict:
    """name without prefix -> (restype, [argtypes]) of every prototype of the header, in its order.  classes: the ctypes.Structure classes
    that may be passed by value or by pointer, found by their class names; by default the header's own structs().  source: the header's
    text (tests)."""
    key = (header, prefix)
    if source is None and key in _signatures:
        return _signatures[key]
    src = re.sub(r"/\*.*?\*/", " ", _source(header) if source is None else source, flags=re.S)
    by_name, sigs = structs(header, prefix, source) if classes is None else {c.__name__: c for c in classes}, {}
    for ret, name, args in re.findall(r"^([\w \t\*]+?)\b%s([a-z_0-9]+)\s*\(([^()]*)\)\s*;" % prefix, src, re.M):
        args = [] if args.strip() == "void" else args.split(",")
        try:
            sigs[name] = (_ctype(ret, by_name, False), [_ctype(a, by_name, True) for a in args])
        except TypeError as e:
            raise TypeError("include/%s: %s%s: %s" % (header, prefix, name, e)) from None
    called = set(re.findall(r"\b%s([a-z_0-9]+)\s*\(" % prefix, src))
    if called != set(sigs):
        raise TypeError("include/%s: not read as prototypes: %s" % (header, ", ".join(prefix + n for n in sorted(called ^ set(sigs)))))
    if source is None:
        _signatures[key] = sigs
    return sigs


_bound = {}


def declare(lib: C.CDLL, header: str, prefix: str, classes=None, symbols: str = None, may_lack=()) -> dict:
    """name without prefix -> the library's function with restype / argtypes set, for every prototype of the header; bound once per
    (library, symbol prefix).  symbols: the prefix the library exports the functions under when it is not the header's (the oracle's dwo_,
    the emulation's dwe_); may_lack: names such a library need not export.  Any other missing symbol is an AttributeError."""
    symbols = symbols or prefix
    key = (lib, symbols)
    if key not in _bound:
        api = {}
        for name, (restype, argtypes) in signatures(header, prefix, classes).items():
            if name in may_lack and not hasattr(lib, symbols + name):
                continue
            f = getattr(lib, symbols + name)
            f.restype, f.argtypes = restype, argtypes
            api[name] = f
        want = constants(header, prefix)[prefix.upper() + "ABI_VERSION"]
        if api["abi_version"]() != want:
            raise DyrosWalkLibraryError("%s: %sabi_version() is %d, include/%s has %d: rebuild the library"
                                        % (getattr(lib, "_name", lib), symbols, api["abi_version"](), header, want))
        _bound[key] = api
    return _bound[key]


def check(api: dict, rc: int):
    """Every entry point returns 0 or an error code, with the message in its ABI's last_error()."""
    if rc != 0:
        raise DyrosWalkLibraryError("%s (code %d)" % (api["last_error"]().decode(), rc))


class Launcher:
    """The base of the classes that launch an ABI's entry points on torch's current stream (recorders.Recorder, model_tensors.ModelTensor):
    self.api is the declared ABI, self._tdev the torch device."""

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self._tdev).cuda_stream

    def _launch(self, entry: str, args: tuple) -> None:
        """One launch on torch's current stream."""
        check(self.api, self.api[entry](*args, self._stream()))
