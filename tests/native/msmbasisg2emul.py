"""ctypes loader of tests/native/libmsmbasisg2emul.so: csrc/msm_basis.h (the bodies of the
fixed-basis MSM) over Fq2, msm.h, msm_group.h, curve.h's jac_add_mixed and the pipeline around
them compiled for the host with g++ (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_basis_g2_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
UNSPLIT = 0xFFFFFFFF
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libmsmbasisg2emul.so")
    return os.path.join(tempfile.gettempdir(), "libmsmbasisg2emul_%d.so" % os.getuid())


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
        L.msm_basis_g2_emul_auto_window.restype = ctypes.c_int
        L.msm_basis_g2_emul_auto_window.argtypes = [ctypes.c_ulonglong]
        _lib = L
    return _lib


def _words(vals):
    k = np.zeros((len(vals), 8), np.uint32)
    for i, v in enumerate(vals):
        for j in range(8):
            k[i, j] = (int(v) >> (32 * j)) & 0xFFFFFFFF
    return k


def table(bases, c):
    """((W(c), nbases, 16) uint64 entries, decoded from the table's lane-half layout
    [x.c0, y.c0 | x.c1, y.c1] into (x, y) images, (nbases,) zero flags) of the emulated build."""
    L = lib()
    p = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 24)
    nb, nw = p.shape[0], 254 // c + 1
    out = np.zeros((nw, nb, 16), np.uint64)
    flags = np.zeros(nb, np.uint8)
    vp = ctypes.c_void_p
    rc = L.msm_basis_g2_emul_table(p.ctypes.data_as(vp), ctypes.c_uint(nb), ctypes.c_int(c), out.ctypes.data_as(vp),
                                flags.ctypes.data_as(vp))
    assert rc == 0, rc
    h = out.reshape(nw, nb, 2, 2, 4)                      # (lane half, x | y, limbs)
    return np.ascontiguousarray(h.transpose(0, 1, 3, 2, 4)).reshape(nw, nb, 16), flags


def msm(bases, scalars, c, cap=0):
    """(the 24-word returned image of sum_{i < len(scalars)} bases[i] * scalars[i] by the emulated
    pipeline over a table of ALL the bases at width c and run cap `cap` (0: the default rule,
    UNSPLIT: never split), {"long": long keys, "levels": fold levels launched}).  scalars:
    canonical integers below r, at most as many as bases."""
    L = lib()
    p = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 24)
    s = _words(list(scalars)) if len(scalars) else np.zeros((1, 8), np.uint32)
    out = np.zeros(24, np.uint64)
    stats = np.zeros(2, np.uint32)
    vp = ctypes.c_void_p
    rc = L.msm_basis_g2_emul_run(p.ctypes.data_as(vp), ctypes.c_uint(p.shape[0]), s.ctypes.data_as(vp),
                              ctypes.c_uint(len(scalars)), ctypes.c_int(c), ctypes.c_uint(cap), out.ctypes.data_as(vp),
                              stats.ctypes.data_as(vp))
    assert rc == 0, rc
    return out, {"long": int(stats[0]), "levels": int(stats[1])}
