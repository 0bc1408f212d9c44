"""ctypes loader of tests/native/libmsmemul.so: csrc/msm.h (the MSM scalar
recoding and bucket keys) compiled for the host with g++ (TEST INFRASTRUCTURE ONLY)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_emul.cpp")
HDR = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc", "msm.h")
_lib = None


def _so_path():
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, "libmsmemul.so")
    return os.path.join(tempfile.gettempdir(), "libmsmemul_%d.so" % os.getuid())


def build(so):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, SRC])


def lib():
    global _lib
    if _lib is None:
        so = _so_path()
        newest = max(os.path.getmtime(SRC), os.path.getmtime(HDR))
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            build(so)
        L = ctypes.CDLL(so)
        for name in ("msm_emul_buckets", "msm_emul_num_keys", "msm_emul_recode_many", "msm_emul_key",
                     "msm_emul_key_weight", "msm_emul_entry", "msm_emul_entry_index"):
            getattr(L, name).restype = ctypes.c_uint
        _lib = L
    return _lib


def recode(scalars, c):
    """signed digits (n, W(c)) int32 of the integer scalars, and the OR of the carries
    out of the top window"""
    L = lib()
    n = len(scalars)
    k = np.zeros((n, 8), np.uint32)
    for i, v in enumerate(scalars):
        for j in range(8):
            k[i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    nw = L.msm_emul_windows(c)
    d = np.zeros((n, nw), np.int32)
    carry = L.msm_emul_recode_many(k.ctypes.data_as(ctypes.c_void_p), n, c, d.ctypes.data_as(ctypes.c_void_p))
    return d, carry
