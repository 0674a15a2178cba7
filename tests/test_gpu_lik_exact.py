"""The fp64 tree of the likelihood kernels — the path of every scan of 4097 .. 28 146 points in the default mode and of every
size with strict_order 0 (host_measure.h:lik_mode) — against the EXACT sum of the reference's float terms
(tests/lik_terms_ref.py, pinned to the oracle in tests/test_lik_terms_cpu.py), at the shapes of tests/lik_exact_cases.py.

likelihood_tiled_body adds G terms per lane and a shuffle tree in double; partial_sum[tile][particle] is then added over every 8th
tile and narrowed to float once — by lik_finalize_kernel behind measure_batch and behind an update of up to 1024 particles, by
lik_pf_partial_kernel (pf_kernels.h; its own tile walk, 64 particles per work-group) in an update of more, and in every rank's
update of a device group. The per-particle, small-scan and one-launch kernels add in double likewise. Every case names the route
it is there for; tests/test_lik_terms_cpu.py checks the name against a restatement of the host's decisions, and this file that
the options those decisions read hold the defaults the restatement assumes. So for every checked particle, with e32 = float32(exact):

    got == e32   or   |float64(got) - exact| <= 0.5 max(spacing(e32), spacing(got)) + n 2^-53 sum |t|
    ratio == float32(count) / float32(n_s)

No number is chosen: half a float ulp for the single narrowing, plus the derived bound of the double additions (~1e-12 of the
sum). On the same inputs at most 0.2 % of a particle's terms are smaller than one float ulp of its sum (asserted on the CPU), so
a work-group that loses or double-counts a term, a tile added twice or not at all, or an evaluation that picks the second-nearest
candidate fails here; the rtol 1e-5 against the reference's float recurrence elsewhere leaves ~100 ulp for them to hide in.
Every case prints its worst error / bound."""
import numpy as np
import pytest

import lik_exact_cases as lc
import lik_terms_ref as lt
from mcl_3dl_amd import capi
from oracle import pyoracle

pytestmark = pytest.mark.gpu
F = np.float32


ALL = lc.CASES + lc.WINDOW
UPDATE_CATEGORY = 3  # MCL3DL_KERNEL_UPDATE: the whole update as one launch


def launch(engine, case):
    """One launch over all the particles of the case through its entry point: (lik, ratio, beam or None)."""
    sc = case.scene()
    beam = None
    stamp = 9100 + ALL.index(case)
    if case.entry.startswith("group"):
        g = capi.Group([0, 0, 0], collective="host")
        try:
            g.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=case.dist_weight)
            g.set_likelihood_params(match_dist_flat=case.flat)
            for k, v in case.options:
                g.set_option(k, v)
            if case.entry == "group-update":
                got = g.measure_update(sc.poses, sc.weights, sc.scan_lik)
                lik, ratio = got["lik"], got["quality"]
            else:
                lik, ratio, _ = g.measure_batch(sc.poses, sc.scan_lik)
        finally:
            g.close()
        return lik, ratio, beam
    # the options the route restatement (lik_exact_cases.route_of) reads are the defaults it assumes
    for k, v in lc.OPTION_DEFAULTS.items():
        assert engine.get_option(k) == v, (k, engine.get_option(k))
    engine.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=case.dist_weight)
    try:
        engine.set_kernel_timing(True)
        engine.reset_kernel_time()
        engine.set_likelihood_params(match_dist_flat=case.flat)
        if case.n_b:
            engine.set_beam_params(num_points=case.n_b)
        for k, v in case.options:
            engine.set_option(k, v)
        if case.entry == "update":
            got = engine.measure_update(sc.poses, sc.weights, sc.scan_lik)
            lik, ratio = got["lik"], got["quality"]
        elif case.n_b:
            lik, ratio, beam = engine.measure_batch(sc.poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
        else:
            lik, ratio, _ = engine.measure_batch(sc.poses, sc.scan_lik)
        # the one route the engine reports itself: the whole update as one launch, or not
        assert (engine.kernel_time(UPDATE_CATEGORY)[1] > 0) == case.route.startswith("one-launch"), case.route
    finally:
        engine.set_kernel_timing(False)
        for k, v in lc.DEFAULTS.items():
            engine.set_option(k, v)
        engine.set_likelihood_params()
        engine.set_beam_params()
    return lik, ratio, beam


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_fp64_tree_is_the_rounded_exact_sum_of_the_reference_s_terms(engine, oracle_kind, case):
    lik, ratio, beam = launch(engine, case)
    assert lik.shape == (case.n_p,) and np.all(np.isfinite(lik))
    idx = case.checked()
    worst, worst_p, rounded, bad = 0.0, -1, 0, []
    for p in idx:
        lst = lc.listing(oracle_kind, case, p)
        lc.check_sharpness(case, lst, p)
        r = lt.error_over_bound(lik[p], lst)
        rounded += lik[p] == F(lst.exact)
        if r > worst:
            worst, worst_p = r, int(p)
        if not (lik[p] == F(lst.exact) or r <= 1.0):
            bad.append((int(p), float(lik[p]), lst.exact, r))
        assert ratio[p] == lt.ratio(lst.count, case.n_s), (case.id, p)
    print("%s: %d particles checked, %d of them float32(exact sum) itself, worst error / bound %.4f (particle %d)"
          % (case.id, len(idx), rounded, worst, worst_p))
    assert not bad, "%s: (particle, got, exact sum, error / bound) %s" % (case.id, bad[:6])
    if beam is not None:  # the merged launch: the beam model's scores are still the oracle's
        sc = case.scene()
        o = lc.oracle(oracle_kind, case)
        o.set_beam_params(pyoracle.BeamParams(num_points=case.n_b))
        want, _ = o.beam_measure(sc.poses[idx], sc.scan_beam, sc.scan_beam_label, sc.origins, threads=4)
        np.testing.assert_array_equal(beam[idx], want)
        assert len(np.unique(beam)) > 1


@pytest.mark.parametrize("case", lc.WINDOW, ids=lambda c: c.id)
def test_either_side_of_the_fp64_window_is_the_reference_s_float_recurrence(engine, oracle_kind, case):
    """4096 and 28 147 points in the default mode: the caller-order float sums, == the oracle. With 4097 and 28 146 among the
    cases above this pins lik_mode's window from both sides."""
    lik, ratio, _ = launch(engine, case)
    sc, idx = case.scene(), case.checked()
    want_lik, want_ratio = lc.oracle(oracle_kind, case).likelihood_measure(sc.poses[idx], sc.scan_lik, threads=4)
    np.testing.assert_array_equal(lik[idx], want_lik)
    np.testing.assert_array_equal(ratio[idx], want_ratio)
