"""tests/long_lived_cases.py on the oracle alone (no GPU): the constraints on the script's order
hold in both directions, every kind the long-lived context is meant to run is there on every
route, the script's sizes and the oracle's work stay within their budgets, and a handful of
the stored expectations agree with a second route through the oracle."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import long_lived_cases as L
from tests import msm_many_cases as M

KINDS = {"pairing_many", "pairing_batch", "miller_loop_batch", "miller_loop_many", "final_exponentiation_many",
         "g2_precompute_many", "g2_prepare", "pairing_prepared_many", "miller_loop_prepared_many", "g2_prepared_destroy",
         "pairing_batch_many", "pairing_batch_prepared_many", "g1_mul_many", "g2_mul_many", "g1_msm", "g2_msm",
         "g1_bases_prepare", "g1_msm_prepared_many", "g1_prepared_destroy", "g1_msm_many", "g1_basis_prepare",
         "g1_msm_basis", "g1_basis_destroy", "g1_group", "g2_group", "fq12_op_many", "gt_pow_many", "fq_sqrt_many",
         "fq2_sqrt_many", "g1_from_compressed_many", "g2_from_compressed_many", "handle_churn",
         "err:miller_loop_batch_zero", "err:products_offsets", "err:prepared_index_host", "err:prepared_index_dev",
         "err:destroyed_handle"}


@pytest.fixture(scope="module")
def passes():
    return L.order(False), L.order(True)


def test_the_order_meets_its_constraints_in_both_directions():
    first, middle, last, draw = L.script()
    assert L.check_order(first, middle, last) == []
    print("order found at draw %d of the generator seeded with %#x" % (draw, L.SEED))
    # and check_order does see a script that breaks them: the units in creation order with one
    # setting never put back, one adjacency lost
    broken = [[s for s in u if not (s["kind"] == "set:msm_min" and s["value"] == 0)] for u in middle]
    broken = [[s for s in u if s["kind"] != "gt_pow_many"] for u in broken]
    bad = L.check_order(first, broken, last)
    assert any("settings left changed" in b for b in bad) and any("gt_pow_many never adjacent" in b for b in bad)


def test_reverse_pass_is_the_middle_reversed(passes):
    fwd, rev = passes
    first, middle, last, _ = L.script()
    nf, nl = len(first), len(last)
    assert [id(s) for s in fwd[:nf]] == [id(s) for s in rev[:nf]] and [id(s) for s in fwd[-nl:]] == [id(s) for s in rev[-nl:]]
    mid_f, mid_r = fwd[nf:-nl], rev[nf:-nl]
    assert len(mid_f) == len(mid_r) and [id(s) for s in mid_f] != [id(s) for s in mid_r]
    assert [id(s) for s in mid_f] == [id(s) for u in middle for s in u]
    # the units come in the opposite order, each with its inner order kept
    at = len(mid_r)
    for u in middle:
        at -= len(u)
        assert [id(s) for s in mid_r[at:at + len(u)]] == [id(s) for s in u]
    assert at == 0


def test_every_kind_on_every_route(passes):
    fwd, _ = passes
    kinds = {s["kind"] for s in fwd if not s["kind"].startswith("set:")}
    assert kinds == KINDS
    count = {k: sum(1 for s in fwd if s["kind"] == k) for k in kinds}
    assert all(v >= 2 for v in count.values()), {k: v for k, v in count.items() if v < 2}
    sizes = lambda kind, **kw: sorted(s["size"] for s in fwd if s["kind"] == kind and all(s.get(k) == v for k, v in kw.items()))  # noqa: E731
    assert {1, 7, 33, L.B_PAIRS, 257} <= set(sizes("pairing_many", route=None))
    assert {7, 33, 257} <= set(sizes("pairing_many", route="throughput"))
    assert {3, 40} <= set(sizes("pairing_batch")) and {3, 40} <= set(sizes("miller_loop_batch"))
    for kind, routes in (("pairing_batch_many", ("wide", "packed", "alone")), ("pairing_batch_prepared_many", ("wide", "packed")),
                         ("g1_msm", ("small", "bucket")), ("g2_msm", ("small", "bucket")), ("g1_msm_many", ("packed", "alone"))):
        assert {s["route"] for s in fwd if s["kind"] == kind} == set(routes), kind
    # prepared pairings with and without an index array
    for kind in ("pairing_prepared_many", "miller_loop_prepared_many"):
        assert {s["idx"] is None for s in fwd if s["kind"] == kind} == {True, False}, kind
    # prepared products mix fresh and prepared terms
    for s in fwd:
        if s["kind"] == "pairing_batch_prepared_many":
            fresh = int((s["qidx"] == L.FRESH).sum())
            assert 0 < fresh < s["size"] and s["q"].shape[0] == fresh
    # a zero row in every final exponentiation; a Miller value inside every wave of powers of 7 or more
    assert all((s["want"][1] == 0).sum() == 1 for s in fwd if s["kind"] == "final_exponentiation_many")
    # the settings: each changed and put back; the passes under msm_run_max(1) and msm_window(2)
    sets = [(s["name"], s["value"]) for s in fwd if s["kind"].startswith("set:")]
    assert {n for n, _ in sets} == set(L.DEFAULTS)
    assert ("msm_run_max", 1) in sets and ("msm_window", 2) in sets and ("fe_wide_max", 0) in sets and ("msm_min", 4096) in sets


def test_sizes_and_budgets(passes):
    fwd, rev = passes
    assert sorted(map(id, fwd)) == sorted(map(id, rev))
    calls = [s for s in fwd if not s["kind"].startswith("set:") and s["size"] > 0]
    print("%d steps in a pass, %d of them calls with data" % (len(fwd), len(calls)))
    assert len(calls) >= 80
    for s in fwd:
        if s["cls"] == "msm":
            assert s["size"] <= 300, L.step_label(s)
        elif s["kind"] in ("pairing_batch_many", "pairing_batch_prepared_many"):
            assert int(np.diff(s["off"].astype(np.int64)).max()) <= 64 and s["size"] <= 257, L.step_label(s)
        else:
            assert s["size"] <= 257, L.step_label(s)
    assert L.oracle_pairings() <= 2000
    made, peak = L.handle_counts(fwd)
    assert made >= 24 and peak == 6
    # the churn steps' handles come from different points
    seen = set()
    for s in fwd:
        if s["kind"] == "handle_churn":
            for grp, key in (("g2", "q"), ("g1p", "bases"), ("basis", "bases")):
                for h in s[grp]:
                    sig = (grp, h[key].tobytes())
                    assert sig not in seen
                    seen.add(sig)
    assert len(seen) == 21


def test_outcome_steps_and_their_followers(passes):
    for steps in passes:
        for a, b in zip(steps, steps[1:]):
            if a["kind"].startswith("err:"):
                assert b["kind"] != a["kind"] and "want" in b and not b["kind"].startswith("err:"), L.step_label(a)
    fwd, _ = passes
    bad = [s for s in fwd if s["kind"] == "err:prepared_index_dev"][0]
    good = [s for s in fwd if s["kind"] == "pairing_prepared_many" and s["size"] == 7][0]
    assert int(bad["idx"][3]) == 3 and not bad["want"][3].any()
    keep = [i for i in range(7) if i != 3]
    assert np.array_equal(bad["want"][keep], good["want"][keep]) and good["want"][3].any()
    for s in fwd:
        if s["kind"] == "err:products_offsets":
            off = s["off"].astype(np.int64)
            assert off[0] != 0 or (np.diff(off) < 0).any()
        if s["kind"] == "err:miller_loop_batch_zero":
            assert O.miller_loop_batch(s["q"], s["p"])[0] != 0


def test_expectations_agree_with_a_second_oracle_route(passes):
    fwd, _ = passes
    by = lambda kind, **kw: [s for s in fwd if s["kind"] == kind and all(s.get(k) == v for k, v in kw.items())]  # noqa: E731
    # product rows against O.pairing_batch on the slices, and against the product of the pairings
    s = by("pairing_batch_many", route="packed")[0]
    off = [int(x) for x in s["off"]]
    for j, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert np.array_equal(s["want"][j], O.pairing_batch(s["p"][a:b], s["q"][a:b], L.NT))
    s = by("pairing_batch", size=3)[0]
    e = O.pairing_many(s["p"], s["q"], L.NT)
    prod = O.binary("orc_fq12_mul", O.binary("orc_fq12_mul", e[0], e[1], 48, 48, 48), e[2], 48, 48, 48)[0]
    assert np.array_equal(s["want"], prod)
    # pairings = the final exponentiation of the Miller values
    s = by("miller_loop_many", size=3)[0]
    fe, rcs = O.final_exponentiation(s["want"])
    assert rcs == [0, 0, 0] and np.array_equal(fe, O.pairing_many(s["p"], s["q"], L.NT))
    # an MSM's value from the segmented helper (one segment of all its terms) and the other way round
    s = by("g1_msm", size=40)[0]
    assert np.array_equal(M.expect(s["p"], s["k"], M.offsets_of([40]))[0], s["want"])
    s = by("g1_msm_many", route="alone")[0]
    off = [int(x) for x in s["off"]]
    from tests import msm_basis_cases as B
    for j, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert np.array_equal(s["want"][j], B.expect(s["p"][a:b], s["k"][a:b]))
    assert max(b - a for a, b in zip(off[:-1], off[1:])) > 8      # the segment above bn_set_msm_many_max(8)
    # a prepared product's rows against the full-q product
    s = by("pairing_batch_prepared_many", route="wide")[0]
    table = by("g2_prepare", name="A")[0]["q"]
    from tests import dev_ordering_cases as D
    assert np.array_equal(s["want"], D.products(s["p"], D.full_q(s["qidx"], table, s["q"]), s["off"]))
    # powers: a mixed wave holds both a pairing output and a Miller value; k = the scalar's image
    s = by("gt_pow_many", size=7)[0]
    cyc = [np.array_equal(O.unary("orc_fq12_cyclotomic_squared", a, 48)[0][0], O.unary("orc_fq12_squared", a, 48)[0][0])
           for a in s["a"]]
    assert any(cyc) and not all(cyc)
    # eq rows: the planted equal pair in another scaling, and unequal ones
    s = by("g1_group", size=17)[0]
    assert s["want"][4][0] == 1 and s["want"][4][1] == 0 and s["want"][4][5] == 0
