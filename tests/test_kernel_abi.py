"""The ctypes signature table of ``ops/_lib.py`` against the C prototypes in ``ops/csrc/*.hip``: same names, same
arity, every argument in the same type class.  A source-text check (no library, no GPU): a ``c_int`` where the C
side takes ``int64_t`` would hand a kernel a truncated row count."""
import ctypes
import glob
import os
import re

from alink_amd.ops import _lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
# C type (qualifiers dropped) -> class; anything with a ``*`` is a pointer, and so is ``hipStream_t`` (HIP's
# ``typedef struct ihipStream_t* hipStream_t``), which als.hip and tree_hist.hip spell out for the stream argument
C_CLASS = {"int": "int", "int64_t": "int64", "float": "float", "double": "double", "uint32_t": "uint32",
           "unsigned": "uint32", "uint64_t": "uint64", "unsigned long long": "uint64", "hipStream_t": "pointer"}
CTYPES_CLASS = {ctypes.c_int: "int", ctypes.c_int64: "int64", ctypes.c_float: "float", ctypes.c_double: "double",
                ctypes.c_uint32: "uint32", ctypes.c_uint64: "uint64", ctypes.c_void_p: "pointer"}
# a column-0 definition: ``int alink_<name>(<parameters>) {``
DEFINITION = re.compile(r"^int (alink_\w+)\s*\(([^)]*)\)\s*\{", re.M)


def _c_class(param: str) -> str:
    """Class of one C parameter declaration (``const float* x``, ``int64_t n``, ``unsigned long long key``)."""
    if "*" in param:
        return "pointer"
    words = [w for w in param.split() if w not in ("const", "volatile")]
    return C_CLASS.get(" ".join(words[:-1]), "unknown type '%s'" % param.strip())     # the last word is the name


def _ctypes_class(t) -> str:
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "pointer"
    return CTYPES_CLASS.get(t, "unknown ctypes type %r" % (t,))


def _prototypes() -> dict:
    protos = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            text = re.sub(r"//[^\n]*", "", f.read())
        for name, params in DEFINITION.findall(text):
            assert name not in protos, f"{name} is defined twice"
            params = params.strip()
            protos[name] = [] if params in ("", "void") else [_c_class(p) for p in params.split(",")]
    return protos


def test_signature_table_matches_the_c_prototypes():
    protos = _prototypes()
    assert len(protos) >= 90, f"the parser found only {len(protos)} exported definitions"
    table = _lib._SIGNATURES
    assert sorted(set(protos) - set(table)) == [], "exported by the sources, missing from _SIGNATURES"
    assert sorted(set(table) - set(protos)) == [], "in _SIGNATURES, not defined by the sources"
    wrong = []
    for name in sorted(protos):
        want, got = protos[name], [_ctypes_class(t) for t in table[name]]
        if len(want) != len(got):
            wrong.append(f"{name}: {len(want)} C parameters, {len(got)} ctypes arguments")
            continue
        wrong += [f"{name} argument {i}: C {w}, ctypes {g}" for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not wrong, "\n".join(wrong)
