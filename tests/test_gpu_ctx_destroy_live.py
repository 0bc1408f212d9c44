"""A context destroyed while its handles are alive: bn_ctx_destroy frees the tables of every
bn_g2_prepared, bn_g1_prepared and bn_g1_basis handle the context still holds (csrc/ctx_mem.h
HandleList), and a context created afterwards is none the worse for it.  Two rounds, each on a
context of its own: one handle of each kind from the first inputs of the churn step of
tests/long_lived_cases.py, each used once against the oracle's stored answer, then the context
destroyed with all three alive."""
import numpy as np
import pytest

from tests import long_lived_cases as L

pytestmark = pytest.mark.gpu


def same(got, want, what):
    assert np.array_equal(np.asarray(got), want), what + ": differs from the oracle"


def test_destroy_with_live_handles_twice():
    from substrate_bn import Context
    s = L._churn(L.pool(), 0)
    g2, g1p, basis = s["g2"][0], s["g1p"][0], s["basis"][0]
    idx = np.arange(2, dtype=np.uint32)
    for rnd in ("first context", "second context"):
        ctx = Context(0)
        a, b, c = ctx.g2_prepare(g2["q"]), ctx.g1_bases_prepare(g1p["bases"]), ctx.g1_basis_prepare(basis["bases"])
        same(ctx.pairing_prepared_many(g2["p"], a, idx), g2["want"], rnd + ": a prepared G2 handle")
        same(ctx.g1_msm_prepared_many(b, g1p["scal"]), g1p["want"], rnd + ": a prepared G1 handle")
        same(ctx.g1_msm_basis(c, basis["k"]), basis["want"], rnd + ": a basis handle")
        rc, ctx._h = ctx._L.bn_ctx_destroy(ctx._h), None  # a, b and c are still alive
        assert rc == 0, rnd + ": bn_ctx_destroy"
