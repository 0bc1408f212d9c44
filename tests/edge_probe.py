"""Child process of tests/test_gpu_edges.py (not collected by pytest).

The product library reads BN254MI_TAIL_FUSED once per process, so the 4,224-term
product of the structured pairs that is exactly one runs here with the variable
set by the parent: with 0 the tail is k_seg_fe1 + k_horner_tree2.  Prints one JSON
line; the test asserts on it.  The oracle is the checker only.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "paritytech-bn_amd"))

from oracle import oracle as O  # noqa: E402
from substrate_bn import _native  # noqa: E402
from tests import edge_vectors as E  # noqa: E402


def main():
    pn, qn = E.one_product_terms(4224)
    ctx = _native.Context(0)
    res = {"n": int(pn.shape[0]), "code": 0, "is_one": False, "bit_exact": False}
    try:
        got = ctx.pairing_batch(pn, qn)
        res["is_one"] = bool(np.array_equal(got, O.canon_to_mont_array([1] + [0] * 11)))
        res["bit_exact"] = bool(np.array_equal(got, O.pairing_batch(pn, qn, nthreads=16)))
    except _native.BnError as e:
        res["code"] = e.code
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
