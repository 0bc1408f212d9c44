"""The counter that stamps the words pairing_batch's one-launch tail and k_fe_ds poll
(csrc/tail_epoch.h: bn_ctx.tail_epoch) on the CPU: tests/native/tail_epoch_main.cpp includes
that header alone, is built with AddressSanitizer + UndefinedBehaviorSanitizer (any report
fails the run) and run as a child process.  Over the wraps 2, 3, 7 (five cycles each) and the
default 2^29 - 1 (three cycles, every step) it checks that the epoch is never 0 and never above
the wrap, that the clear of the two stamped buffers is flagged on every return to 1 and nowhere
else, that a fresh context starts at 1 with no clear, that the default sequence is the launch
sites' earlier rule, and the range $BN254MI_TAIL_EPOCH_WRAP accepts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "tail_epoch_main.cpp")
HDR = os.path.join(ROOT, "paritytech-bn_amd", "csrc", "tail_epoch.h")
EXE = os.path.join(NATIVE, "tail_epoch_main.bin")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_tail_epoch_under_asan_ubsan():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tail epoch ok" in r.stdout
