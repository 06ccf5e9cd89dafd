"""What the per-feature CPU tests share about the C ABI: the header text and the one question each of them asks about the
symbols its feature added.  Types, argument order and struct layouts are test_abi_cpu.py's, for every symbol at once."""
import os
import re

from consistencytta_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
with open(os.path.join(INCLUDE, "ctta.h")) as _f:
    HEADER = _f.read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)           # the header without its comments


def declared_symbols():
    """Every ctta_* name the header follows with `(`, found without the package's header reader."""
    return sorted(set(re.findall(r"\b(ctta_[a-z0-9_]+)\s*\(", CODE)))


def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def assert_bound(names, lib=None):
    """Each name is declared in include/ctta.h, has a ctypes signature and is exported by the built library."""
    lib = lib or built_lib()
    declared = declared_symbols()
    for name in names:
        assert name in declared, "%s is not declared in include/ctta.h" % name
        assert name in N.SIGNATURES, "%s has no ctypes signature" % name
        assert hasattr(lib, name), "libctta_hip.so does not export %s" % name
        assert list(getattr(lib, name).argtypes) == N.SIGNATURES[name][1], "%s is not bound" % name
