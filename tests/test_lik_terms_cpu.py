"""What tests/test_gpu_lik_exact.py stands on, checked without a GPU: tests/lik_terms_ref.py restates the reference's likelihood
terms (its float cumulative sum IS Oracle.likelihood_measure, bit for bit, on every particle the GPU test checks — the plain-C
port always, the reference's own sources where they are built), every case of tests/lik_exact_cases.py is sharp, and the gate is
shown to be sharp once: a lost term, a doubled term and the reference's own float recurrence all fall outside it."""
import math

import numpy as np
import pytest

import lik_exact_cases as lc
import lik_terms_ref as lt
from oracle import pyoracle

KINDS = [k for k in ("port", "ref") if pyoracle.available(k)]
F, D = np.float32, np.float64


@pytest.mark.parametrize("case", lc.CASES + lc.WINDOW, ids=lambda c: c.id)
def test_restatement_is_the_oracle_and_the_case_is_sharp(case):
    assert "port" in KINDS
    sc, idx = case.scene(), case.checked()
    for kind in KINDS:
        want_lik, want_ratio = lc.oracle(kind, case).likelihood_measure(sc.poses[idx], sc.scan_lik, threads=4)
        worst_share, least = 0.0, None
        for k, p in enumerate(idx):
            lst = lc.listing(kind, case, p)
            assert len(lst.terms) == case.n_s and lst.terms.dtype == F
            assert lt.float_recurrence(lst.terms) == want_lik[k], (kind, p)
            assert lt.ratio(lst.count, case.n_s) == want_ratio[k], (kind, p)
            assert lst.exact == lst.sum_abs  # (no term is negative)
            worst_share = max(worst_share, lc.check_sharpness(case, lst, p))
            least = lst.count if least is None else min(least, lst.count)
        print("%s, %s: %d particles, at most %.3g %% of the terms below one ulp of the sum, at least %d matched points"
              % (case.id, kind, len(idx), 100.0 * worst_share, least))


def test_checked_particles_cover_the_groups_and_the_finalize_boundaries():
    for case in lc.CASES:
        idx = set(case.checked().tolist())
        assert min(case.n_p, 24) <= len(idx) <= lc.MAX_CHECKED
        g = case.group_size() if case.tiled else {"small": {8: 32, 32: 8}.get(case.n_s)}.get(case.route.split("/")[0], 1)
        for lo, hi in case.shards():
            n = hi - lo
            want = set(range(min(g, n))) | set(range((n - 1) // g * g, n)) | {i for i in (31, 32, 63, 64) if i < n}
            if case.route.endswith("pf-tail"):  # lik_pf_partial_kernel: 64 particles per work-group; either side of the first
                want |= {63, 64, n - 1}         # boundary, the last particle and (one context: 48 to check) the whole last one
                if case.entry == "update":
                    want |= set(range((n - 1) // 64 * 64, n))
            assert {lo + i for i in want} <= idx, case.id
    # every value the cases vary appears at least twice
    for values in ([c.jitter for c in lc.CASES], [c.dist_weight for c in lc.CASES], [c.flat for c in lc.CASES]):
        assert all(values.count(v) >= 2 for v in set(values))
    assert {c.flat for c in lc.CASES} == {0.05, 0.0, 0.18}
    assert {c.opts.get("lik_group", 0) for c in lc.TILED if (c.n_p, c.n_s) == (300, 6143)} == {0, 4, 8, 16, 32}


@pytest.mark.parametrize("case", lc.CASES + lc.WINDOW, ids=lambda c: c.id)
def test_case_takes_the_route_it_is_there_for(case):
    """host_measure.h:lik_mode / lik_small_applies / lik_particle_block / launch_update_small and host_pf.h:pf_form /
    pf_takes_tiles restated over the option defaults (lik_exact_cases.route_of): a case that drifted onto another kernel fails here."""
    assert lc.route_of(case) == case.route


def test_every_route_has_a_case():
    routes = {c.route for c in lc.CASES}
    assert routes == {"tiled/fp64/finalize", "tiled/fp64/pf-tail", "small/fp64", "particle64/fp64", "particle256/fp64",
                      "particle1024/fp64", "one-launch1024/fp64"}
    tails = [c for c in lc.CASES if c.route == "tiled/fp64/pf-tail"]
    assert {c.entry for c in tails} == {"update", "group-update"}
    # the tail's tile walk: with and without a last trip of one tile behind the paired slices (n_tiles % 8 in 1 .. 4, else)
    assert {((c.n_s + 255) // 256) % 8 for c in tails} >= {0, 5}


def test_bound_is_the_worst_case_of_double_summation():
    """Sequential, pairwise and 8-way strided double sums of a listing's terms (the associations the kernels use) stay inside
    bound(); the bound itself is ~1e-12 of the sum, five orders of magnitude below half a float ulp."""
    case = lc.BENCH_SCAN
    lst = lc.listing("port", case, 0)
    t = lst.terms.astype(D)
    b = lt.bound(lst.count, lst.sum_abs)
    seq = 0.0
    for x in t.tolist():
        seq += x
    tree = t.copy()
    while len(tree) > 1:
        if len(tree) % 2:
            tree = np.concatenate([tree, [0.0]])
        tree = tree[0::2] + tree[1::2]
    strided = 0.0
    for s in [sum(t[k::8].tolist()) for k in range(8)]:
        strided += s
    for got in (seq, float(tree[0]), strided, float(np.sum(t))):
        assert abs(got - lst.exact) <= b
    assert b < 1e-11 * lst.exact and b < 1e-4 * 0.5 * float(np.spacing(F(lst.exact)))


def test_the_gate_sees_a_lost_term_a_doubled_term_and_the_reference_s_own_rounding():
    case = lc.BENCH_SCAN
    idx = case.checked()
    ref_fails = 0
    for p in idx:
        lst = lc.listing("port", case, p)
        # the correctly rounded exact sum passes, and so does the double sum in scan order narrowed once
        assert lt.error_over_bound(F(lst.exact), lst) <= 1.0
        assert lt.error_over_bound(F(float(np.sum(lst.terms.astype(D)))), lst) <= 1.0
        ulp = float(np.spacing(F(lst.exact)))
        above = lst.terms[lst.terms.astype(D) > ulp]
        small = float(above.min())  # the smallest term above one ulp of the sum
        for wrong in (lst.exact - small, lst.exact + small):  # ... left out, added twice
            assert lt.error_over_bound(F(wrong), lst) > 1.0, (p, small, ulp)
        # the reference's float recurrence taken as if it were the engine's result
        ref_fails += lt.error_over_bound(lt.float_recurrence(lst.terms), lst) > 1.0
    print("%s: the reference's own float recurrence misses the gate on %d of %d checked particles" % (case.id, ref_fails, len(idx)))
    assert ref_fails >= 1


def test_tolerance_is_half_an_ulp_plus_the_bound():
    lst = lt.Listing(np.array([0.75, 0.5, 0.25], F), 3, 1.5, 1.5)
    assert lt.bound(3, 1.5) == 3 * 2.0 ** -53 * 1.5
    assert lt.tolerance(F(1.5), lst) == 0.5 * 2.0 ** -23 + lt.bound(3, 1.5)
    assert lt.error_over_bound(F(1.5), lst) == 0.0
    assert lt.error_over_bound(np.nextafter(F(1.5), F(2)), lst) > 1.9
    # a sum exactly between two floats may round either way
    half = lt.Listing(lst.terms, 3, 1.5 + 2.0 ** -24, 1.5 + 2.0 ** -24)
    assert lt.error_over_bound(F(1.5), half) <= 1.0 and lt.error_over_bound(np.nextafter(F(1.5), F(2)), half) <= 1.0
    # at a power of two the wider of the two spacings counts
    edge = lt.Listing(lst.terms, 3, 2.0 - 2.0 ** -25, 2.0)
    assert lt.tolerance(F(2.0), edge) == 0.5 * 2.0 ** -22 + lt.bound(3, 2.0)
    assert math.isfinite(lt.error_over_bound(F(0.0), lt.Listing(np.zeros(1, F), 0, 0.0, 0.0)))
