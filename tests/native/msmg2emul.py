"""ctypes loader of tests/native/libmsmg2emul.so: csrc/msm_group.h (the group-law
bodies of the bucket MSM) and the pipeline around them compiled for the host with g++
(TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_g2_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libmsmg2emul.so")
    return os.path.join(tempfile.gettempdir(), "libmsmg2emul_%d.so" % os.getuid())


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
        L.msm_g2_emul_segment.restype = ctypes.c_uint
        _lib = L
    return _lib


def msm(group, points, scalars, c):
    """The returned image (12 or 24 words) of sum points[i] * scalars[i] by the emulated
    bucket pipeline at window width c.  points: (n, 12) / (n, 24) uint64 images; scalars:
    canonical integers below r."""
    L = lib()
    width = {"g1": 12, "g2": 24}[group]
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, width)
    n = p.shape[0]
    assert len(scalars) == n
    k = np.zeros((n, 8), np.uint32)
    for i, v in enumerate(scalars):
        for j in range(8):
            k[i, j] = (int(v) >> (32 * j)) & 0xFFFFFFFF
    out = np.zeros(width, np.uint64)
    vp = ctypes.c_void_p
    rc = getattr(L, "msm_g2_emul_" + group)(p.ctypes.data_as(vp), k.ctypes.data_as(vp), ctypes.c_uint(n), ctypes.c_int(c),
                                            out.ctypes.data_as(vp))
    assert rc == 0, rc
    return out
