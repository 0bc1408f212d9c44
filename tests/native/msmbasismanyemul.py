"""ctypes loader of tests/native/libmsmbasismanyemul.so: csrc/msm_basis_many.h (the index
arithmetic of the batched fixed-basis MSM), msm_basis.h, msm.h, msm_group.h and the batched
pipeline around them compiled for the host with g++ (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_basis_many_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
UNSPLIT = 0xFFFFFFFF
ARRAYS = ("keys", "sorted", "buckets", "run_a", "run_b", "parts")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libmsmbasismanyemul.so")
    return os.path.join(tempfile.gettempdir(), "libmsmbasismanyemul_%d.so" % os.getuid())


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
        L.msm_basis_many_emul_set.restype = ctypes.c_ulonglong
        L.msm_basis_many_emul_set.argtypes = [ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_ulonglong,
                                              ctypes.c_ulonglong]
        _lib = L
    return _lib


def set_size(m, n, c, max_keys=0, forced=0):
    """msm_basis_many_set: the vectors of a launch set."""
    return int(lib().msm_basis_many_emul_set(m, n, c, max_keys, forced))


def msm(bases, rows, n, c, cap=0, forced=0):
    """((m, 12) returned images of sum_{i < n} bases[i] * rows[j][i], j < m, by the emulated
    batched pipeline over a table of ALL the bases at width c, run cap `cap` (0: the default
    rule, UNSPLIT: never split) and `forced` vectors per launch set (0: the default); and
    {"levels", "S", "sets", "long": per vector, "touched" / "alloc": per array}).  rows: m
    lists of canonical integers below 2^256, each of the same length k_stride >= n."""
    L = lib()
    p = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
    m = len(rows)
    stride = len(rows[0]) if m else n
    assert all(len(r) == stride for r in rows)
    s = np.zeros((max(m * stride, 1), 8), np.uint32)
    for j, r in enumerate(rows):
        for i, v in enumerate(r):
            for w in range(8):
                s[j * stride + i, w] = (int(v) >> (32 * w)) & 0xFFFFFFFF
    out = np.zeros((max(m, 1), 12), np.uint64)
    nlong = np.zeros(max(m, 1), np.uint32)
    stats = np.zeros(3, np.uint32)
    touched = np.zeros(6, np.uint64)
    alloc = np.zeros(6, np.uint64)
    vp = ctypes.c_void_p
    rc = L.msm_basis_many_emul_run(p.ctypes.data_as(vp), ctypes.c_uint(p.shape[0]), s.ctypes.data_as(vp),
                                   ctypes.c_ulonglong(stride), ctypes.c_uint(m), ctypes.c_uint(n), ctypes.c_int(c),
                                   ctypes.c_uint(cap), ctypes.c_uint(forced), out.ctypes.data_as(vp),
                                   nlong.ctypes.data_as(vp), stats.ctypes.data_as(vp), touched.ctypes.data_as(vp),
                                   alloc.ctypes.data_as(vp))
    assert rc == 0, rc
    return out[:m], {"levels": int(stats[0]), "S": int(stats[1]), "sets": int(stats[2]),
                     "long": [int(x) for x in nlong[:m]],
                     "touched": dict(zip(ARRAYS, (int(x) for x in touched))),
                     "alloc": dict(zip(ARRAYS, (int(x) for x in alloc)))}
