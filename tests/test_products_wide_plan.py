"""The wide path's part of the pairing products' host-side planning (csrc/products_plan.h,
DESIGN.md 6d) on the CPU: tests/native/products_wide_plan_main.cpp includes that header
alone, is built with AddressSanitizer + UndefinedBehaviorSanitizer (any report fails the run)
and run as a child process.  It checks that without the wide limits the plan is, field for
field, the plan of the rules before the path (over the offset arrays of
tests/test_products_plan.py and seeded random ones), the routing rule of both product calls on
each side of each of its conditions, the cuts of the wide sets at W terms and at 2^18
products, and the gather words of a mixed fresh and prepared call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "products_wide_plan_main.cpp")
HDR = os.path.join(ROOT, "paritytech-bn_amd", "csrc", "products_plan.h")
EXE = os.path.join(NATIVE, "products_wide_plan_main.bin")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_products_wide_plan_under_asan_ubsan():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "products wide plan ok" in r.stdout
