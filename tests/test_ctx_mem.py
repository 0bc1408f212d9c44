"""The types that own a context's device and pinned memory (csrc/ctx_mem.h: DevBuf, PinBuf,
grow_together, UploadChannel, Fence, HandleList) on the CPU: tests/native/ctx_mem_main.cpp
includes csrc/ctx.h against a stand-in HIP runtime (tests/native/fakehip: allocations backed by
malloc and counted, the k-th made to fail on request), is built with AddressSanitizer +
UndefinedBehaviorSanitizer (any report fails the run) and run as a child process.  It checks
the grow rule (no call at or below the capacity; drain, floor and free above it), a failing
allocation in a grow and in each of the workspace's four, the channel and its fence (the wait
only while a copy is pending, before a grow; one event), the handle list (lookups that never
read the handle, drain before free, a dropped build) and that a context with every buffer
grown and a handle of each kind leaves nothing live when destroyed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "paritytech-bn_amd", "csrc")
SRC = os.path.join(NATIVE, "ctx_mem_main.cpp")
FAKE = os.path.join(NATIVE, "fakehip")
DEPS = [SRC, os.path.join(FAKE, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "bn254mi.h")] + [
    os.path.join(CSRC, h) for h in ("ctx.h", "ctx_mem.h", "tail_epoch.h")]
EXE = os.path.join(NATIVE, "ctx_mem_main.bin")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_ctx_mem_under_asan_ubsan():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-I", FAKE, "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ctx mem ok" in r.stdout
