"""float_chain.h:seq_sum_wave ON THE DEVICE, through the four kernels whose bits it decides — pf_fused_kernel (float_order),
pf_strict_sum_kernel, update_small_kernel and the per-particle likelihood kernel's LDS row — against the plain float32 loop, at
the inputs where the wavefront form leaves its shortcut: rounding ties, equal terms, wild magnitudes, NaN, infinities,
negative terms, -0, denormals, every lane as the first one in trouble (tests/float_chain_cases.py;
tests/test_float_chain_cpu.py states which of them reach a wavefront pass, a clean one, one with trouble). And pf::measure's
restore rule (`sum > 0.0` as a float, pf.h:262-278) in every form pf::measure takes: NaN, +inf, 0, a negative sum, an overflowing one.

The yardstick is tests/pf_measure_ref.py, never another user of seq_sum_wave. Weights are compared as bit patterns: with hundreds
of quotients by the same float, a sum that is off by one ulp cannot pass."""
import math

import numpy as np
import pytest

import float_chain_cases as fc
import pf_measure_ref as pr
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def eng():
    """A context of this module's own: its options, map and parameters are no other test's business."""
    e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scene():
    """The reference's default scan sizes (96 + 3 points) for up to 4097 particles."""
    return make_scene(n=91, n_p=4097, n_s=96, n_b=3, seed=411)


def configure(obj, sc, stamp):
    obj.set_map(sc.map_xyz, sc.map_label, stamp=stamp, dist_weight=(1.0, 1.0, 5.0))
    obj.set_likelihood_params()
    obj.set_beam_params(num_points=3)


def float_order(strict_order, n):
    """host_pf.h:pf_float_order — does pf::measure on one GPU add the weights as the reference does?"""
    return strict_order == 1 or (strict_order == 2 and n <= fc.FUSED_MAX)


def assert_bits(got, want, msg):
    got, want = np.asarray(got, F), np.asarray(want, F)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="%s: NaN pattern" % (msg,))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok], err_msg=str(msg))


def assert_entropy(got, wn, s, restored, msg):
    """NaN where restored; where alive and the sum is finite, within pf_measure_ref.entropy's bound (derived there, not
    measured on a kernel)."""
    if restored:
        assert math.isnan(got["entropy"]), msg
    elif math.isfinite(float(s)):
        H, bound = pr.entropy(wn, s)
        assert abs(got["entropy"] - H) <= bound, (msg, got["entropy"], H, bound)


def assert_is_reference(got, ref, msg):
    """A float-order form: the flag and every weight are the restatement's, bit for bit."""
    assert got["restored"] == ref["restored"], (msg, float(ref["sum"]))
    assert_bits(got["weights"], ref["weights"], msg)
    assert_entropy(got, ref["wn"], ref["sum"], ref["restored"], msg)


def assert_tree_form(got, w0, ref, msg):
    """An fp64-tree form: it divides by the exact sum rounded to float where the reference divides by its recurrence's float, so
    the flag follows from that sum, the weights are untouched when restored, and alive they are 0 / NaN under an infinite sum or
    wn / sum otherwise, within 2^-22: one ulp of the divisor (the tree's double is within 2^-50 of the exact sum, so its float
    is at most the neighbour of the exact sum's) plus the quotient's own rounding on either side."""
    wn = ref["wn"]
    with np.errstate(all="ignore"):
        if np.all(np.isfinite(wn)):
            exact = math.fsum(wn.astype(np.float64))
            sum_f = F(exact)
        else:
            exact = None
            sum_f = F(np.sum(wn.astype(np.float64)))   # NaN, or an infinity whose sign the terms agree on
        restored = not sum_f > 0.0
        assert got["restored"] == restored, (msg, float(sum_f))
        if restored:
            assert_bits(got["weights"], w0, msg)
            assert math.isnan(got["entropy"]), msg
        elif np.isinf(sum_f):
            assert_bits(got["weights"], (wn / sum_f).astype(F), msg)
        else:
            np.testing.assert_allclose(got["weights"], wn.astype(np.float64) / float(sum_f), rtol=2.0 ** -22, atol=2.0 ** -149,
                                       err_msg=str(msg))
            assert_entropy(got, wn, exact, False, msg)


# ---- (a) every family x size through pf::measure with w0 = 1 and lik = t: wn is t in every bit ---------------------------
A_CASES = [(family, n) for family in fc.FAMILIES[:5] for n in fc.SIZES] + [("every_lane", n) for n in fc.EVERY_LANE_SIZES]


def forms_a(n):
    """(strict_order, pf_fused): strict_order 1 at every size — pf_fused_kernel up to 1024 particles, pf_strict_sum_kernel +
    pf_apply_kernel with pf_fused 0 and beyond; the default strict_order 2 on either side of 1024."""
    if n <= fc.FUSED_MAX:
        return [(1, 1), (1, 0), (2, 1), (2, 0)]
    return [(1, 1), (2, 1)]


@pytest.mark.parametrize("family,n", A_CASES, ids=["%s-%d" % c for c in A_CASES])
def test_float_order_forms_are_the_serial_loop(eng, family, n):
    cases = fc.family_cases(family, n)
    w0 = np.ones(n, F)
    refs = [pr.measure(w0, t) for _, t in cases]
    for (name, t), ref in zip(cases, refs):
        assert fc.same_bits(ref["wn"], t)   # (the products by 1 change no bit: the kernels add exactly the family's terms)
    try:
        for strict_order, pf_fused in forms_a(n):
            eng.set_option("strict_order", strict_order)
            eng.set_option("pf_fused", pf_fused)
            for (name, t), ref in zip(cases, refs):
                got = eng.pf_measure(w0, t)
                msg = (name, "strict_order %d pf_fused %d" % (strict_order, pf_fused))
                if float_order(strict_order, n):
                    assert_is_reference(got, ref, msg)
                else:
                    assert_tree_form(got, w0, ref, msg)
    finally:
        eng.set_option("strict_order", 2)
        eng.set_option("pf_fused", 1)


# ---- (b) the restore rule in every form --------------------------------------------------------------------------------
B_SIZES = (64, 300, 1024, 1025, 4097)


def restore_cases(n):
    """{name: (lik, restored as the case intends)} for w0 = 1."""
    small = (fc.weights(n) * F(0.01)).astype(F)   # adds up to about 0.3
    out = {}
    for tag, pos in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        t = fc.weights(n)
        t[pos] = np.nan
        out["nan-" + tag] = (t, True)
    t = fc.weights(n)
    t[n // 3] = np.inf
    out["inf"] = (t, False)
    out["zeros"] = (np.zeros(n, F), True)
    t = small.copy()
    t[n // 2] = F(-1.0)
    out["negative-sum"] = (t, True)
    # non-negative finite terms whose total exceeds 1e39 (n >= 64 terms of at least 1e38): the float sum is +inf, the update is alive
    out["overflow"] = (((F(0.5) + fc.weights(n) * F(n / 45.0)) * F(2e38)).astype(F), False)
    return out


@pytest.mark.parametrize("n", B_SIZES)
def test_restore_rule_in_every_form_of_pf_measure(eng, n):
    """strict_order 0 / 1 / 2 x pf_fused 0 / 1: the fused kernel with the fp64 tree and with the float recurrence, partial +
    self-reducing apply, partial / reduce / strict sum / apply. (The negative sum is -1 + 0.3 in any association, so the
    fp64-tree forms take that case too; they get no other negative term.)"""
    w0 = np.ones(n, F)
    cases = restore_cases(n)
    refs = {name: pr.measure(w0, t) for name, (t, _) in cases.items()}
    for name, (t, restored) in cases.items():
        assert refs[name]["restored"] is restored, name
        assert np.all(np.isfinite(t)) or name.startswith(("nan", "inf")), name
    assert np.isinf(refs["overflow"]["sum"]) and np.all(refs["overflow"]["weights"] == 0)
    assert math.fsum(cases["overflow"][0].astype(np.float64)) > 1e39
    try:
        for strict_order in (0, 1, 2):
            for pf_fused in (0, 1):
                eng.set_option("strict_order", strict_order)
                eng.set_option("pf_fused", pf_fused)
                for name, (t, restored) in cases.items():
                    got = eng.pf_measure(w0, t)
                    msg = (name, n, "strict_order %d pf_fused %d" % (strict_order, pf_fused))
                    if float_order(strict_order, n):
                        assert_is_reference(got, refs[name], msg)
                    else:
                        assert_tree_form(got, w0, refs[name], msg)
                    # stated once more without the helpers: the flag, weights untouched when restored, 0 / NaN when alive
                    assert got["restored"] is restored, msg
                    if restored:
                        assert_bits(got["weights"], w0, msg)
                    else:
                        with np.errstate(all="ignore"):
                            assert_bits(got["weights"], np.where(np.isinf(t), F(np.nan), F(0)), msg)
    finally:
        eng.set_option("strict_order", 2)
        eng.set_option("pf_fused", 1)


def test_restore_rule_through_the_sharded_protocol(eng, scene):
    """A one-device group with direct_single 0: partial / reduce / (strict sum) / all-reduce / apply apart. A group has no
    pf::measure of its own, so the adversarial factor travels as `extra` of a measurement update at the reference's default scan
    sizes; what is expected is the restatement applied to the likelihoods and beam scores the call itself returns."""
    sc = scene
    configure(eng, sc, 9400)
    g = capi.Group((0,))
    try:
        configure(g, sc, 9400)
        g.set_option("direct_single", 0)
        for n in B_SIZES:
            poses, w0 = sc.poses[:n], np.ones(n, F)
            lik0, _, beam0 = eng.measure_batch(poses, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins)
            prod = (beam0 * lik0).astype(F)
            top = int(np.argmax(prod))
            assert prod[top] > 0 and np.all(np.isfinite(prod))
            extras = {}
            for tag, pos in (("first", 0), ("middle", n // 2), ("last", n - 1)):
                e = fc.weights(n)
                e[pos] = np.nan
                extras["nan-" + tag] = (e, True)
            e = fc.weights(n)
            e[top] = np.inf
            extras["inf"] = (e, False)
            extras["zeros"] = (np.zeros(n, F), True)
            e = np.full(n, F(1e-9))
            e[top] = F(-1.0)
            extras["negative-sum"] = (e, True)
            # every product at most 2e38 and finite, the largest of them 2e38: the sum overflows when a second particle is
            # within a factor of three of the best one (asserted below on the restatement)
            extras["overflow"] = (np.full(n, F(2e38) / prod[top], F), False)
            for strict_order in (0, 1, 2):
                g.set_option("strict_order", strict_order)
                for name, (extra, restored) in extras.items():
                    got = g.measure_update(poses, w0, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins, extra=extra)
                    msg = (name, n, "strict_order %d" % strict_order)
                    # (strict_order 0 adds the likelihood terms in an fp64 tree: a few ulp from lik0, which only chose `top`)
                    np.testing.assert_allclose(got["lik"], lik0, rtol=1e-5)
                    assert_bits(got["beam"], beam0, msg)
                    ref = pr.measure(w0, got["lik"], got["beam"], extra)
                    assert ref["restored"] is restored, msg   # (a condition on the scene: the case is what its name says)
                    if name == "overflow":
                        assert np.all(np.isfinite(ref["wn"])) and np.isinf(ref["sum"]), msg
                    if float_order(strict_order, n):
                        assert_is_reference(got, ref, msg)
                    else:
                        assert_tree_form(got, w0, ref, msg)
                    assert got["restored"] is restored, msg
                    if restored:
                        assert_bits(got["weights"], w0, msg)
    finally:
        g.close()


# ---- (c) update_small_kernel: the whole update in one launch, the weights added in the dynamic LDS row -----------------
def update_small_inputs(n):
    """[(name, w0, extra)] from the weights, ties, equal and specials families."""
    out = [("weights x ties", fc.weights(n), fc.ties(n)), ("equal x weights", fc.equal(n), fc.weights(n)),
           ("ties x equal", fc.ties(n), fc.equal(n))]
    for tag, t in fc.specials(n):
        out.append(("weights x specials %s" % tag, fc.weights(n), t))
    for tag, t in fc.specials(n)[::5]:
        out.append(("specials %s x equal" % tag, t, fc.equal(n)))
    return out


@pytest.mark.parametrize("n_p,small_max", [(257, 512), (300, 512), (512, 512), (769, 8192), (1000, 8192)])
def test_update_small_kernel_adds_the_weights_as_the_serial_loop(eng, scene, n_p, small_max):
    sc = scene
    configure(eng, sc, 9400)
    try:
        eng.set_option("update_small", 1)
        eng.set_option("update_small_max", small_max)
        for name, w0, extra in update_small_inputs(n_p):
            got = eng.measure_update(sc.poses[:n_p], w0, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins, extra=extra)
            assert np.count_nonzero(got["lik"]) > 0 and np.all(np.isfinite(got["lik"]))
            ref = pr.measure(w0, got["lik"], got["beam"], extra)
            assert_is_reference(got, ref, (name, n_p))
    finally:
        eng.set_option("update_small", 1)
        eng.set_option("update_small_max", 512)


# ---- (d) the per-particle likelihood kernel's LDS row on terms known exactly by construction ---------------------------
LATTICE = 8                                   # map points at the integers 0 .. 7 on every axis
TRANSLATIONS = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 1]], F)   # identity rotations: every particle sees the same terms


def lattice_scan(n_s, grid_bits, k_max):
    """(scan, terms): scan points whose terms are exact. A point at a lattice point plus dx = k 2^-grid_bits along x (0 <= dx <=
    0.25) has one neighbour in reach of match_dist_min = 0.75 (the next one is at 1 - dx >= 0.75, and the radius test is strict),
    d^2 = dx^2 and its root are exact (k < 2^12), and with match_dist_flat = 0 and match_weight = 1 the term is 0.75 - dx, exact
    as well (every coordinate stays below 8: multiples of 2^-20 fit a float there). A point at half-integer offsets on all three
    axes is sqrt(0.75) from eight map points: no match, the term +0. k is odd, or odd times a power of two: an odd multiple
    of half an ulp — a rounding tie — in the binade whose half ulp is that power of two times 2^-grid_bits, a multiple of the ulp
    in the binades below and a plain rounding in those above."""
    rng = np.random.default_rng([n_s, grid_bits])
    cell = rng.integers(1, 5, (n_s, 3)).astype(F)   # 1 .. 4: the particles' translations keep it inside the map
    shift = rng.integers(0, int(math.log2(k_max)) + 1, n_s)         # the power of two, then an odd factor that keeps k <= k_max
    k = (2 * (rng.integers(0, 1 << 20, n_s) % (((k_max >> shift) + 1) // 2)) + 1) << shift
    k[rng.integers(0, 40, n_s) == 0] = 0            # on the map point itself: the largest term
    dx = np.ldexp(k.astype(F), -grid_bits).astype(F)
    assert np.all(dx <= 0.25) and np.all(k <= k_max) and k_max < 4096
    half = rng.integers(0, 32, n_s) == 0
    scan = cell.copy()
    scan[:, 0] += dx
    scan[half] = cell[half] + F(0.5)
    terms = np.where(half, F(0), F(0.75) - dx).astype(F)
    assert np.array_equal(scan[~half, 0].astype(np.float64), cell[~half, 0].astype(np.float64) + dx[~half].astype(np.float64))
    return scan, terms, int(np.count_nonzero(~half))


@pytest.fixture(scope="module")
def lattice_engine():
    e = capi.Engine(0)
    ax = np.arange(LATTICE, dtype=F)
    e.set_map(np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3), None, stamp=9500)
    e.set_likelihood_params(match_dist_min=0.75, match_dist_flat=0.0, match_weight=1.0)
    e.set_beam_params(num_points=1)
    yield e
    e.close()


@pytest.mark.parametrize("grid_bits,k_max", [(12, 1024), (20, 4095)], ids=["2^-12", "2^-20"])
@pytest.mark.parametrize("n_s", [257, 769, 2049, 6000])
def test_likelihood_row_on_exact_terms(lattice_engine, n_s, grid_bits, k_max):
    """Three particles: launch_measure's plan (host_measure.h:lik_mode) gives fewer than four particles the per-particle kernel at
    every scan size, with the caller-order LDS row up to 12 288 points under the default strict_order — read back as lik_exact.
    Steps of 2^-12 are what the sizes were chosen for: below 4096 every sum of them is exact, and 6000 points with small dx
    cross 4096, where odd k are rounding ties. Steps of 2^-20 tie in every binade from [16, 32) up, so every size rounds."""
    e = lattice_engine
    if grid_bits == 12 and n_s == 6000:
        k_max = 64   # terms of at least 0.734: the sum passes 4096 several hundred terms before the end
    scan, terms, matched = lattice_scan(n_s, grid_bits, k_max)
    want = fc.serial_sum(terms)
    if grid_bits == 20 or n_s == 6000:   # a condition on the inputs: the recurrence rounds, it is not an exact sum in disguise
        assert float(want) != math.fsum(terms.astype(np.float64))
    poses = np.zeros((len(TRANSLATIONS), 7), F)
    poses[:, :3] = TRANSLATIONS
    poses[:, 6] = 1.0
    scan_robot = scan - TRANSLATIONS[0]
    lik, ratio, _ = e.measure_batch(poses, scan_robot)
    assert e.get_option("lik_exact") == 1
    for p in range(len(poses)):
        assert_bits(lik[p:p + 1], [want], ("measure_batch", n_s, grid_bits, p))
    np.testing.assert_array_equal(ratio, F(matched) / F(n_s))
    upd = e.measure_update(poses, np.ones(len(poses), F), scan_robot)   # the one-launch update runs the same row
    for p in range(len(poses)):
        assert_bits(upd["lik"][p:p + 1], [want], ("measure_update", n_s, grid_bits, p))
    np.testing.assert_array_equal(upd["quality"], F(matched) / F(n_s))
    assert_is_reference(upd, pr.measure(np.ones(len(poses), F), upd["lik"], upd["beam"]), ("measure_update", n_s, grid_bits))
