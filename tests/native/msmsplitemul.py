"""ctypes loader of tests/native/libmsmsplitemul.so: the split of overlong bucket runs
(csrc/msm.h's plan, csrc/msm_group.h's bodies) and the pipeline around it compiled for the
host with g++ (TEST INFRASTRUCTURE ONLY).  build_main() builds the same source as a
stand-alone program, optionally under sanitizers."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msm_split_emul.cpp")
CSRC = os.path.join(HERE, "..", "..", "paritytech-bn_amd", "csrc")
UNSPLIT = 0xFFFFFFFF
_lib = None


def _path(name):
    if os.access(HERE, os.W_OK):
        return os.path.join(HERE, name)
    base, ext = os.path.splitext(name)
    return os.path.join(tempfile.gettempdir(), "%s_%d%s" % (base, os.getuid(), ext))


def _stale(out):
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")))
    newest = max(newest, os.path.getmtime(SRC))
    return not os.path.exists(out) or os.path.getmtime(out) < newest


def build(so):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])


def build_main(sanitize=True):
    """The stand-alone program (its own main: the plan checks over generated histograms);
    returns its path."""
    exe = _path("msm_split_emul_main_san" if sanitize else "msm_split_emul_main")
    if _stale(exe):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DMSM_SPLIT_EMUL_MAIN"] + flags + ["-o", exe, SRC])
    return exe


def lib():
    global _lib
    if _lib is None:
        so = _path("libmsmsplitemul.so")
        if _stale(so):
            build(so)
        L = ctypes.CDLL(so)
        for name in ("msm_split_emul_cap_default", "msm_split_emul_level_slots", "msm_split_emul_fan",
                     "msm_split_emul_run_min"):
            getattr(L, name).restype = ctypes.c_uint
        _lib = L
    return _lib


def plan_check(counts, L, n, nent_bound=None):
    """(rc, info): rc 0 when every invariant of the plan holds over the histogram `counts`
    for a call of n terms, else the negative number of the first one violated
    (msm_split_emul.cpp plan_check); info = [long keys, the level at which the last key
    finished, level-0 slots in use, the host's levels, the host's level-0 bound]."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    info = np.zeros(5, np.uint32)
    bound = int(c.sum()) if nent_bound is None else nent_bound
    vp = ctypes.c_void_p
    rc = lib().msm_split_emul_plan_check(c.ctypes.data_as(vp), ctypes.c_uint(c.size), ctypes.c_uint(L), ctypes.c_uint(n),
                                         ctypes.c_uint(bound), info.ctypes.data_as(vp))
    return rc, [int(v) for v in info]


def msm(group, points, scalars, c, cap):
    """(image, long keys, fold levels) of sum points[i] * scalars[i] by the emulated bucket
    pipeline at window width c and run cap `cap` (0: the default rule; UNSPLIT: never split).
    points: (n, 12) / (n, 24) uint64 images; scalars: canonical integers below r."""
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
    stats = np.zeros(2, np.uint32)
    vp = ctypes.c_void_p
    rc = getattr(L, "msm_split_emul_" + group)(p.ctypes.data_as(vp), k.ctypes.data_as(vp), ctypes.c_uint(n), ctypes.c_int(c),
                                               ctypes.c_uint(cap), out.ctypes.data_as(vp), stats.ctypes.data_as(vp))
    assert rc == 0, rc
    return out, int(stats[0]), int(stats[1])
