"""ctypes loader of tests/native/libmsmmanyemul.so: csrc/msm_many.h (the bodies of
bn_g1_msm_many's packed path), csrc/msm_many_plan.h and the pipeline around them compiled
for the host with g++ (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_many_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libmsmmanyemul.so")
    return os.path.join(tempfile.gettempdir(), "libmsmmanyemul_%d.so" % os.getuid())


def build(so):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])


def lib():
    global _lib
    if _lib is None:
        so = _so_path()
        newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")))
        newest = max(newest, os.path.getmtime(SRC))
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            build(so)
        L = ctypes.CDLL(so)
        L.msm_many_emul_digit_roundtrip.restype = ctypes.c_int
        L.msm_many_emul_digit_roundtrip.argtypes = [ctypes.c_int]
        L.msm_many_emul_run.restype = ctypes.c_int
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        L.msm_many_emul_run.argtypes = [vp, vp, vp, sz, ctypes.c_int, ctypes.c_uint, sz, sz, vp]
        _lib = L
    return _lib


def _words(vals):
    k = np.zeros((len(vals), 8), np.uint32)
    for i, v in enumerate(vals):
        for j in range(8):
            k[i, j] = (int(v) >> (32 * j)) & 0xFFFFFFFF
    return k


def msm_many(points, scalars, offsets, c, unit, chunk=1 << 17, lanes=1 << 17):
    """The (m, 12) returned images of the segments' sums by the emulated pipeline at window
    width c, `unit` terms per unit (0: automatic at `lanes`) and launch sets of `chunk` terms.
    points: (n, 12) uint64 images; scalars: n canonical integers below r; offsets: m + 1."""
    L = lib()
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    m = off.shape[0] - 1
    assert p.shape[0] == len(scalars) == int(off[-1])
    s = _words(scalars)
    out = np.zeros((max(m, 1), 12), np.uint64)
    vp = ctypes.c_void_p
    rc = L.msm_many_emul_run(p.ctypes.data_as(vp), s.ctypes.data_as(vp), off.ctypes.data_as(vp), m, c, unit, chunk,
                             lanes, out.ctypes.data_as(vp))
    assert rc == 0, rc
    return out[:m]
