"""ctypes loader of tests/native/libproductsemul.so: the loop body of k_miller_products
(csrc/pairing.h miller_product_scaled) compiled for the host with g++ in the one-lane
layout (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "products_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libproductsemul.so")
    return os.path.join(tempfile.gettempdir(), "libproductsemul_%d.so" % os.getuid())


def build(so):
    # -O1: the host checks (BN_HOST_CHECKS: the fold bounds) stay in
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
        L.pe_miller_product.restype = ctypes.c_int
        _lib = L
    return _lib


def miller_product(p_affine, q_affine, dead=None, iterate=None):
    """The Miller value (48 words) of one product by the kernel's loop body.
    p_affine: (K, 8) uint64 (x, y) images, q_affine: (K, 16) uint64 (x.c0, x.c1, y.c0, y.c1);
    dead: K flags, a set one gives that pair the line one; iterate: pairs the loop runs over
    (default K; more is the padding to the wave's largest product).  Returns (value, lines
    fetched)."""
    p = np.ascontiguousarray(p_affine, dtype=np.uint64).reshape(-1, 8)
    q = np.ascontiguousarray(q_affine, dtype=np.uint64).reshape(-1, 16)
    k = p.shape[0]
    assert q.shape[0] == k
    pairs = np.ascontiguousarray(np.concatenate([p, q], axis=1))
    flags = np.zeros(max(k, 1), np.uint8)
    if dead is not None:
        flags[:k] = np.asarray(dead, dtype=np.uint8)
    out = np.zeros(48, np.uint64)
    vp = ctypes.c_void_p
    fetched = lib().pe_miller_product(pairs.ctypes.data_as(vp), ctypes.c_int(k), flags.ctypes.data_as(vp),
                                      ctypes.c_int(k if iterate is None else iterate), out.ctypes.data_as(vp))
    return out, fetched
