"""The interface of the pairing products' wide path that needs no device:
bn_set_products_wide_max and bn_get_products_routes in the header, in the built library and in
the Python mirror's symbol table, and the mirror's methods and argument checks on a stub
library."""
import os
import re
import subprocess

import numpy as np
import pytest

from substrate_bn import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bn254mi.h")
LIB = os.path.join(ROOT, "paritytech-bn_amd", "libbn254mi.so")
NEW = ("bn_set_products_wide_max", "bn_get_products_routes")


def test_header_declares_the_two_calls():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+bn_set_products_wide_max\s*\(\s*bn_ctx\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+bn_get_products_routes\s*\(\s*bn_ctx\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\[\s*3\s*\]\s*\)\s*;", text)
    # the reader sits with the measurement calls, behind bn_get_phase_times
    assert text.index("bn_get_phase_times(") < text.index("bn_get_products_routes(") < text.index("---- workspace ----")


def test_built_library_exports_the_two_calls():
    assert os.path.exists(LIB), "libbn254mi.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in defined, name


def test_native_mirror_lists_the_two_calls():
    for name in NEW:
        assert name in _native.EXPORTS
    for m in ("set_products_wide_max", "products_routes"):
        assert callable(getattr(_native.Context, m))


class _Lib:
    """Stands in for the native library: records the calls, fills the counts."""

    def __init__(self, rc=_native.BN_OK):
        self.calls = []
        self.rc = rc

    def bn_set_products_wide_max(self, h, terms):
        self.calls.append(("set", terms))
        return self.rc

    def bn_get_products_routes(self, h, counts):
        self.calls.append(("get",))
        import ctypes
        a = ctypes.cast(counts, ctypes.POINTER(ctypes.c_size_t))
        a[0], a[1], a[2] = 5, 1 << 40, 7
        return self.rc

    def bn_last_error(self, h):
        return b"stub"


def _ctx(rc=_native.BN_OK):
    c = _native.Context.__new__(_native.Context)
    c._h = None
    c._L = _Lib(rc)
    return c


def test_setter_passes_integers_through():
    c = _ctx()
    c.set_products_wide_max(0)
    c.set_products_wide_max(4096)
    c.set_products_wide_max(np.int64(12))
    c.set_products_wide_max((1 << 64) - 1)
    assert c._L.calls == [("set", 0), ("set", 4096), ("set", 12), ("set", (1 << 64) - 1)]
    assert all(type(t) is int for _, t in c._L.calls)


@pytest.mark.parametrize("bad", [-1, 1 << 64, 2.0, "8", None, True, [4]])
def test_setter_refuses_what_is_not_a_term_count(bad):
    c = _ctx()
    with pytest.raises(ValueError):
        c.set_products_wide_max(bad)
    assert c._L.calls == []


def test_routes_are_three_python_integers():
    c = _ctx()
    r = c.products_routes()
    assert r == (5, 1 << 40, 7) and all(type(v) is int for v in r)
    assert c._L.calls == [("get",)]


def test_native_errors_raise():
    c = _ctx(_native.BN_ERR_INVALID_ARGUMENT)
    with pytest.raises(_native.BnError) as e:
        c.set_products_wide_max(1)
    assert e.value.code == _native.BN_ERR_INVALID_ARGUMENT
    with pytest.raises(_native.BnError):
        c.products_routes()
