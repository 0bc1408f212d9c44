"""The host-side planning of the pairing products (csrc/products_plan.h: the planner of
bn_pairing_batch_many and bn_pairing_batch_prepared_many, the refusals of their control
arrays, the offset and map words of a launch set) on the CPU: tests/native/
products_plan_main.cpp includes that header alone, is built with AddressSanitizer +
UndefinedBehaviorSanitizer (any report fails the run) and run as a child process.  It
checks the plans of fixed offset arrays (products_min, products_chunk, a product above the
lane maximum, empty products, more than one launch set of products), the map words of one
set, each refusal's message, and the plan's invariants over 200 seeded random arrays."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "products_plan_main.cpp")
HDR = os.path.join(ROOT, "paritytech-bn_amd", "csrc", "products_plan.h")
EXE = os.path.join(NATIVE, "products_plan_main.bin")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_products_plan_under_asan_ubsan():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "products plan ok" in r.stdout
