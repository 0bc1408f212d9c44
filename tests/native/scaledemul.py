"""ctypes wrapper of tests/native/libscaledemul.so: the pairing on scaled inputs
compiled for the host from the engine's device headers (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libscaledemul.so")
SRC = os.path.join(HERE, "scaled_emul.cpp")
_lib = None


def build():
    # -O1: the host checks (BN_HOST_CHECKS) stay in; at -O0 one pairing takes seconds
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DBN_HOST_CHECKS", "-fPIC", "-shared", "-o", SO, SRC])


def lib():
    global _lib
    if _lib is None:
        hdr_dir = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
        newest = max(os.path.getmtime(os.path.join(hdr_dir, f)) for f in os.listdir(hdr_dir))
        newest = max(newest, os.path.getmtime(SRC))
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            build()
        _lib = ctypes.CDLL(SO)
        _lib.se_pairing_scaled.restype = ctypes.c_int
    return _lib


def pairing_scaled(p, q):
    """p: (12,) uint64 Jacobian G1 image, q: (24,) uint64 Jacobian G2 image -> ((48,) uint64 Gt
    image, skip)"""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(12)
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(24)
    out = np.zeros(48, dtype=np.uint64)
    skip = lib().se_pairing_scaled(p.ctypes.data_as(ctypes.c_void_p), q.ctypes.data_as(ctypes.c_void_p),
                                   out.ctypes.data_as(ctypes.c_void_p))
    return out, skip
