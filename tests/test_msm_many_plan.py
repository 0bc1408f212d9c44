"""The host-side planning of bn_g1_msm_many (csrc/msm_many_plan.h: the refusals of the
offsets, the launch sets, the units of every segment, the words a set's kernels read) on the
CPU: tests/native/msm_many_plan_main.cpp includes that header alone, is built with
AddressSanitizer + UndefinedBehaviorSanitizer (any report fails the run) and run as a child
process.  It checks each refusal's message (decreasing offsets, offsets[0] != 0, n and m
above 2^26, m checked before the array is read), the unit cuts for lengths 0, 1, T - 1, T,
T + 1, 64 T, 64 T + 1 and 4096 (every term in exactly one unit, at most 64 units per
segment, at most 64 terms per unit), the set cuts at segment boundaries under a forced small
chunk, the routing of segments over the max to the alone path, and the plan's invariants
over 200 seeded random arrays."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "msm_many_plan_main.cpp")
HDR = os.path.join(ROOT, "paritytech-bn_amd", "csrc", "msm_many_plan.h")
EXE = os.path.join(NATIVE, "msm_many_plan_main.bin")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_msm_many_plan_under_asan_ubsan():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "msm many plan ok" in r.stdout
