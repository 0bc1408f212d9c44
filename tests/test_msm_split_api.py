"""The run cap of the bucket MSM (bn_set_msm_run_max) in the Python mirror, without a
device: the export, the mirror method, the "never split" value and the header's text."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bn254mi.h")


def test_native_mirror_lists_the_setter():
    from substrate_bn import _native
    assert "bn_set_msm_run_max" in _native.EXPORTS
    assert callable(getattr(_native.Context, "set_msm_run_max"))


def test_unsplit_is_the_headers_value():
    from substrate_bn import _native
    assert _native.MSM_RUN_UNSPLIT == ctypes.c_size_t(-1).value
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"#define\s+BN_MSM_RUN_UNSPLIT\s+\(\(size_t\)-1\)", text)
    assert re.search(r"int\s+bn_set_msm_run_max\(bn_ctx\*\s*ctx,\s*size_t\s+entries\);", text)
    assert "No value changes a result" in text
