"""ctypes loader of tests/native/libproductspreparedemul.so: one product of
bn_pairing_batch_prepared_many on the host (csrc/pairing.h prepared_line_scaled and
miller_product_scaled, g++, the one-lane layout; TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "products_prepared_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
REGION_B = 1 << 31
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libproductspreparedemul.so")
    return os.path.join(tempfile.gettempdir(), "libproductspreparedemul_%d.so" % os.getuid())


def build(so):
    # -O1: the host checks (BN_HOST_CHECKS: the fold bounds, which abort) stay in
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DBN_HOST_CHECKS", "-fPIC", "-shared", "-o", so, SRC])


def lib():
    global _lib
    if _lib is None:
        so = _so_path()
        newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")))
        newest = max(newest, os.path.getmtime(SRC))
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            build(so)
        L = ctypes.CDLL(so)
        L.ppe_miller_product.restype = ctypes.c_int
        _lib = L
    return _lib


def miller_product(terms, table_coeffs, dead=None, iterate=None):
    """The Miller value (48 words) of one product and the number of lines the loop fetched.
    terms, in term order: ("fresh", p_affine (8 uint64: x, y), q_affine (16 uint64)) or
    ("prepared", p_jacobian (12 uint64), index into table_coeffs ((nq, 87, 24) uint64: the
    reference's coefficients of the prepared points, as a bn_g2_prepared table holds them)).
    dead: one flag per term, a set one gives that term the line one; iterate: terms the loop
    runs over (default all; more is the padding to the wave's largest product)."""
    table = np.ascontiguousarray(table_coeffs, dtype=np.uint64).reshape(-1, 87, 24)
    fresh, pp, pidx, tmap = [], [], [], []
    for kind, p, q in terms:
        if kind == "fresh":
            tmap.append(len(fresh))
            fresh.append(np.concatenate([np.asarray(p, np.uint64).reshape(8), np.asarray(q, np.uint64).reshape(16)]))
        else:
            tmap.append(REGION_B | len(pp))
            pp.append(np.asarray(p, np.uint64).reshape(12))
            pidx.append(int(q))
    k = len(tmap)
    fa = np.ascontiguousarray(np.stack(fresh)) if fresh else np.zeros((1, 24), np.uint64)
    pa = np.ascontiguousarray(np.stack(pp)) if pp else np.zeros((1, 12), np.uint64)
    ix = np.array(pidx + [0], np.uint32)
    mp = np.array(tmap + [0], np.uint32)
    flags = np.zeros(k + 1, np.uint8)
    if dead is not None:
        flags[:k] = np.asarray(dead, dtype=np.uint8)
    out = np.zeros(48, np.uint64)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    fetched = lib().ppe_miller_product(fa.ctypes.data_as(vp), ci(len(fresh)), table.ctypes.data_as(vp), ci(table.shape[0]),
                                       pa.ctypes.data_as(vp), ix.ctypes.data_as(vp), ci(len(pp)), mp.ctypes.data_as(vp),
                                       ci(k), flags.ctypes.data_as(vp), ci(k if iterate is None else iterate),
                                       out.ctypes.data_as(vp))
    assert fetched >= 0, "a map word outside its region"
    return out, fetched
