"""ctypes loader of tests/native/libpreparedemul.so: the loop body of k_pairing_prepared
(csrc/pairing.h miller_prepared) compiled for the host with g++ in the one-lane layout
(TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "prepared_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libpreparedemul.so")
    return os.path.join(tempfile.gettempdir(), "libpreparedemul_%d.so" % os.getuid())


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
        L.pp_miller_prepared.restype = ctypes.c_int
        _lib = L
    return _lib


def miller_prepared(q_affine, p, gt_form):
    """The Miller value (48 words) of miller_prepared over the lines of the affine G2 point
    q_affine (16 uint64: x.c0, x.c1, y.c0, y.c1) and the number of lines fetched.
    gt_form False: p's first 8 words are the affine (x, y) of P.  gt_form True: p is the
    Jacobian image (12 uint64) and the lines are scaled by Z^3, Y, X Z."""
    q = np.ascontiguousarray(q_affine, dtype=np.uint64).reshape(16)
    pj = np.zeros(12, np.uint64)
    src = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1)
    pj[:src.shape[0]] = src
    out = np.zeros(48, np.uint64)
    vp = ctypes.c_void_p
    fetched = lib().pp_miller_prepared(q.ctypes.data_as(vp), pj.ctypes.data_as(vp), ctypes.c_int(1 if gt_form else 0),
                                       out.ctypes.data_as(vp))
    return out, fetched
