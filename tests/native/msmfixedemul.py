"""ctypes loader of tests/native/libmsmfixedemul.so: csrc/msm_fixed.h (the bodies of the
prepared-bases MSM), curve.h's jac_add_mixed and the pipeline around them compiled for the
host with g++ (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_fixed_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libmsmfixedemul.so")
    return os.path.join(tempfile.gettempdir(), "libmsmfixedemul_%d.so" % os.getuid())


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
        L.msm_fixed_emul_entries.restype = ctypes.c_ulonglong
        L.msm_fixed_emul_entries.argtypes = [ctypes.c_ulonglong, ctypes.c_int]
        L.msm_fixed_emul_auto_lanes.restype = ctypes.c_uint
        L.msm_fixed_emul_auto_lanes.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_int]
        _lib = L
    return _lib


def _words(vals):
    k = np.zeros((len(vals), 8), np.uint32)
    for i, v in enumerate(vals):
        for j in range(8):
            k[i, j] = (int(v) >> (32 * j)) & 0xFFFFFFFF
    return k


def msm_many(bases, scalars, c, lanes):
    """The (m, 12) returned images of sum_b bases[b] * scalars[j][b] by the emulated
    pipeline at window width c and `lanes` lanes per output.  bases: (k, 12) uint64 images;
    scalars: m rows of k canonical integers below r."""
    L = lib()
    p = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
    k, m = p.shape[0], len(scalars)
    assert all(len(row) == k for row in scalars)
    s = _words([v for row in scalars for v in row])
    out = np.zeros((m, 12), np.uint64)
    vp = ctypes.c_void_p
    rc = L.msm_fixed_emul_run(p.ctypes.data_as(vp), ctypes.c_uint(k), s.ctypes.data_as(vp), ctypes.c_uint(m),
                              ctypes.c_int(c), ctypes.c_uint(lanes), out.ctypes.data_as(vp))
    assert rc == 0, rc
    return out


def add_mixed(acc, entry_xy, neg=False):
    """jac_add_mixed(acc, x, [-]y) as a 12-word Jacobian image.  acc: a G1 image; entry_xy:
    the 8 words (x, y) of a normalized point."""
    L = lib()
    a = np.ascontiguousarray(acc, dtype=np.uint64).reshape(12)
    e = np.ascontiguousarray(entry_xy, dtype=np.uint64).reshape(8)
    out = np.zeros(12, np.uint64)
    vp = ctypes.c_void_p
    L.msm_fixed_emul_add_mixed(a.ctypes.data_as(vp), e.ctypes.data_as(vp), ctypes.c_int(1 if neg else 0),
                               out.ctypes.data_as(vp))
    return out
