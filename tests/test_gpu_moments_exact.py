"""The particle reductions behind every scan — pf::measure's sums, expectationBiased / max / maxBiased, covariance
(pf_partial_kernel, pf_apply_kernel, pf_moments_kernel, pf_moments_jump_bias_kernel, pf_covariance_kernel and their reduce kernels)
— against EXACT sums of the reference's float terms (tests/moments_ref.py, itself checked against the oracle in
tests/test_moments_ref_cpu.py), at every size where the code takes another path: one wavefront, one work-group, the grid cap of
1024 x 256 particles and the grid-stride trip past it, shard bounds, subsets.

The kernels add in fp64, so a sum may differ from the exact one by n * 2^-53 * sum |t| (moments_ref.sum_bound; the fifteen
covariance sums that involve a device atan2f / asinf get moments_ref.cov_budget on top). Particles that carry 32 times the mean
weight sit at every index where a loop bound could be off by one; losing any of them moves a sum by thousands of bounds (asserted
on the CPU before the GPU is asked). The host arithmetic behind the sums is asked for bit for bit. Every comparison prints
error / bound."""
import numpy as np
import pytest

import landmark_ref as lr
import moments_ref as mo
from mcl_3dl_amd import capi

pytestmark = pytest.mark.gpu
F, D, CAP = mo.F, mo.D, mo.CAP


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def record(engine, size, call):
    """`call(rec)` writes a shard record of `size` doubles into device memory; returned as a numpy array. The record starts out as
    NaN, so an entry the library does not write shows."""
    import torch
    rec = torch.full((size,), float("nan"), dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    call(rec)
    engine.synchronize()
    return rec.cpu().numpy()


def within(what, got, want, bound, terms=None):
    """|got - want| <= bound per sum; printed with the error and the bound relative to sum |t| (the scale rounding errors have;
    |want| itself where no terms are given)."""
    got, want, bound = np.asarray(got, D), np.asarray(want, D), np.asarray(bound, D)
    scale = np.abs(want) if terms is None else np.abs(np.asarray(terms).astype(D)).sum(axis=0)
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        rel, rel_bound = np.where(scale > 0, err / scale, 0.0), np.where(scale > 0, bound / scale, 0.0)
    print("%s: error / bound %.3g (error %.3g, bound %.3g of sum |t|)" % (what, ratio.max(), rel.max(), rel_bound.max()))
    assert np.all(ratio <= 1.0), (what, ratio)


def moments_record(engine, d_pose, d_w, d_bias, n):
    return record(engine, 16, lambda rec: engine.moments_partial_device(d_pose, d_w, d_bias, n, rec))


def same_expectation(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    assert tuple(a[1:]) == tuple(b[1:])


# ---- the moments record ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mo.SIZES)
def test_moments_record_against_exact_sums(engine, n):
    case = mo.scene_case(n)
    case.check(moments=True, covariance=False)
    d_pose, d_w, d_bias = dev(case.pose7), dev(case.w), dev(case.bias)
    for biased in (False, True):
        exact, bound, im, ib = case.moments(biased)
        terms = case.moment_bounds(biased)[0]
        rec = moments_record(engine, d_pose, d_w, d_bias if biased else None, n)
        within("n %d%s: ten sums" % (n, " biased" if biased else ""), rec[:10], exact, bound, terms)
        assert rec[10] == float(case.w[im]) and rec[11] == im and rec[12] == float(terms[ib, 0]) and rec[13] == ib
        assert rec[14] == 0.0 and rec[15] == 0.0
        fin = engine.moments_finish(rec)
        want_mean, want_total = mo.moments_finish(rec[:10])
        np.testing.assert_array_equal(fin[0], want_mean)
        assert fin[1:] == (want_total, im, ib)
        same_expectation(engine.expectation_device(d_pose, d_w, d_bias if biased else None, n), fin)
        same_expectation(engine.expectation(case.pose7, case.w, case.bias if biased else None), fin)


def test_first_maximum_across_wavefronts_work_groups_and_the_grid_cap(engine):
    """The four-way tie of tests/test_gpu_moments.py spread out: 17 and CAP + 17 are the SAME thread's first and second grid-stride
    trip, 81 another wavefront of its work-group, 300 another work-group, CAP - 1 the last particle of the first trip, CAP + 273
    another work-group's second trip. The reference keeps the first maximum (strict <); the bias hands it on one by one."""
    n = CAP + 600
    ties = [17, 81, 300, CAP - 1, CAP + 17, CAP + 273]
    poses = mo.scene_poses(n, seed=3)
    w = np.full(n, 0.001, F)
    w[ties] = 0.05
    d_pose, d_w = dev(poses), dev(w)
    for k in range(len(ties)):
        bias = np.ones(n, F)
        bias[ties[:k]] = 0.5  # the first k of the tied particles fall behind
        _, im, ib = mo.moment_terms(poses, w, bias)
        assert (im, ib) == (17, ties[k])
        rec = moments_record(engine, d_pose, d_w, dev(bias), n)
        assert (rec[11], rec[13]) == (17, ties[k]) and rec[10] == float(F(0.05)) and rec[12] == float(F(0.05))
        assert engine.expectation(poses, w, bias)[2:] == (17, ties[k])
    # an equal maximum in the second trip alone against one in the first, either way round in the work-group order
    for a, b in ((CAP - 1, CAP), (1023 * 256 + 5, CAP + 2)):
        w2 = np.full(n, 0.001, F)
        w2[[a, b]] = 0.05
        assert engine.expectation(poses, w2)[2:] == (a, a)


# ---- shards ----------------------------------------------------------------------------------------------------------------------
def cuts():
    n = mo.SHARD_N
    out = []
    for world in (2, 3, 8):
        lo = [capi.group_shard(n, world, r)[0] for r in range(world)]
        out.append(("group_shard-%d" % world, lo + [n]))
    out.append(("one-particle-shard", [0, 1000, 1001, n]))
    out.append(("shard-from-the-cap", [0, CAP, n]))
    third = capi.group_shard(n, 3, 1)[0]
    out.append(("empty-first", [0, 0, third, n]))
    out.append(("empty-middle", [0, third, third, n]))
    out.append(("empty-last", [0, third, n, n]))
    return out


@pytest.mark.parametrize("name,cut", cuts(), ids=[c[0] for c in cuts()])
def test_shard_records_combine_to_the_exact_sums(engine, name, cut):
    case = mo.shard_case()
    case.check()
    n = case.n
    d_pose, d_w, d_bias = dev(case.pose7), dev(case.w), dev(case.bias)
    shards = list(zip(cut[:-1], cut[1:]))
    assert shards[0][0] == 0 and shards[-1][1] == n and all(lo <= hi for lo, hi in shards)
    offsets = [lo for lo, _ in shards]
    for biased in (False, True):
        exact, _, im, ib = case.moments(biased)
        terms = case.moment_bounds(biased)[0]
        assert im == mo.SHARD_TIE[0] and ib == (mo.SHARD_TIE[1] if biased else mo.SHARD_TIE[0])
        recs = [moments_record(engine, d_pose[lo:hi], d_w[lo:hi], d_bias[lo:hi] if biased else None, hi - lo) for lo, hi in shards]
        bound = sum(mo.sum_bound(terms[lo:hi]) for lo, hi in shards)
        total = np.zeros(10, D)
        for (lo, hi), rec in zip(shards, recs):
            if hi == lo:  # the record the device group writes for a rank without particles
                np.testing.assert_array_equal(rec, [0.0] * 10 + [-1.0, 0.0, -1.0, 0.0, 0.0, 0.0])
            total = total + rec[:10]  # (rank order, as mcl3dl_hip_moments_finish adds)
        within("%s%s: ten sums over the shards" % (name, " biased" if biased else ""), total, exact, bound, terms)
        fin = engine.moments_finish(np.stack(recs), offsets)
        want_mean, want_total = mo.moments_finish(total)
        np.testing.assert_array_equal(fin[0], want_mean)
        assert fin[1:] == (want_total, im, ib)  # global indices; the maximum tied across two shards goes to the earlier one
        if name.startswith("empty"):  # an empty shard changes nothing, wherever it stands
            kept = [(r, o) for r, o, (lo, hi) in zip(recs, offsets, shards) if hi > lo]
            same_expectation(engine.moments_finish(np.stack([r for r, _ in kept]), [o for _, o in kept]), fin)
    with pytest.raises(capi.EngineError, match="error -3"):  # the single-shot call divides by the sum: still an error
        engine.expectation_device(d_pose[:0], d_w[:0], None, 0)
    # the covariance the same way: 22 sums per shard, added on the host
    cterms, cbound = case.cov_bounds()
    cexact, _ = case.covariance()
    crecs = [record(engine, 22, lambda rec: engine.covariance_partial_device(d_pose[lo:hi], d_w[lo:hi], hi - lo, case.mean7, rec))
             for lo, hi in shards]
    total = np.zeros(22, D)
    for rec in crecs:
        total = total + rec
    bound = sum(mo.sum_bound(cterms[lo:hi]) for lo, hi in shards) + (cbound - mo.sum_bound(cterms))  # + the angle budget
    within("%s: position sums and sum w over the shards" % name, total[mo.POSITION_SUMS], cexact[mo.POSITION_SUMS],
           bound[mo.POSITION_SUMS], cterms[:, mo.POSITION_SUMS])
    within("%s: angle sums over the shards" % name, total[mo.ANGLE_SUMS], cexact[mo.ANGLE_SUMS], bound[mo.ANGLE_SUMS],
           cterms[:, mo.ANGLE_SUMS])
    np.testing.assert_array_equal(engine.covariance_finish(total), mo.covariance_finish(total))


# ---- the covariance record -------------------------------------------------------------------------------------------------------
COV_CASES = [c for c in mo.CASES if c[3] and c[0] not in ("jump-bias", "shards")]


@pytest.mark.parametrize("name,build", [c[:2] for c in COV_CASES], ids=[c[0] for c in COV_CASES])
def test_covariance_record_against_exact_sums(engine, name, build):
    case = build()
    case.check(moments=False, covariance=True)
    exact, bound = case.covariance()
    assert np.all(bound[mo.POSITION_SUMS] == mo.sum_bound(case.cov_bounds()[0])[mo.POSITION_SUMS])  # no budget there
    d_pose, d_w = dev(case.pose7), dev(case.w)
    d_sub = None if case.subset is None else dev(case.subset)
    n_sub = 0 if case.subset is None else len(case.subset)
    rec = record(engine, 22, lambda r: engine.covariance_partial_device(d_pose, d_w, case.n, case.mean7, r, d_sub, n_sub))
    terms = case.cov_bounds()[0]
    within("%s: position sums and sum w" % name, rec[mo.POSITION_SUMS], exact[mo.POSITION_SUMS], bound[mo.POSITION_SUMS],
           terms[:, mo.POSITION_SUMS])
    within("%s: angle sums" % name, rec[mo.ANGLE_SUMS], exact[mo.ANGLE_SUMS], bound[mo.ANGLE_SUMS], terms[:, mo.ANGLE_SUMS])
    cov = engine.covariance_finish(rec)
    np.testing.assert_array_equal(cov, mo.covariance_finish(rec))
    np.testing.assert_array_equal(cov, cov.T)
    np.testing.assert_array_equal(engine.covariance_device(d_pose, d_w, case.n, case.mean7, d_sub, n_sub), cov)
    np.testing.assert_array_equal(engine.covariance(case.pose7, case.w, case.mean7, subset=case.subset), cov)
    if name in ("yaw-wrap", "roll-wrap"):
        a = 5 if name == "yaw-wrap" else 3
        assert 0.02 < cov[a, a] < 0.08  # ~0.2^2, not ~pi^2: the differences were wrapped


# ---- the jump bias and the device group ----------------------------------------------------------------------------------------
def one_ulp(what, got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    ulps = np.abs(got.astype(D) - want.astype(D)) / np.spacing(np.abs(want)).astype(D)
    print("%s: %.3g float ulp" % (what, ulps.max()))
    assert np.all(ulps <= 1.0), (what, got, want)


def group_ids():
    import test_gpu_landmark_bias as lb
    return lb.CONFIGS, lb.IDS


@pytest.mark.parametrize("cfg", group_ids()[0], ids=group_ids()[1])
def test_jump_bias_and_group_reductions_past_the_grid_cap(engine, cfg):
    import test_gpu_landmark_bias as lb
    case = mo.jump_case()
    case.check()
    n, st, w = case.n, case.state13, case.w
    g = lb.group(cfg)
    try:
        g.upload_state(st, w)
        mean, total, im, ib, bias = g.expectation_jump_bias(lb.PREV, lb.VAR_DIST, lb.VAR_ANG, fetch_bias=True)
        cov = g.covariance(mean)
    finally:
        g.close()
    # the reference over the bias the device formed (its own accuracy is tests/test_gpu_landmark_bias.py's subject)
    _, _, ang, _ = lr.jump_bias(st, lb.PREV, lb.VAR_DIST, lb.VAR_ANG, host=False, parts=True)
    lb.assert_rel(bias, case.bias, lr.jump_bias_bound(ang, lb.VAR_ANG))
    terms, wim, wib = mo.moment_terms(case.pose7, w, bias)
    exact, bound = mo.exact_sums(terms), mo.sum_bound(terms)
    assert (im, ib) == (wim, wib)
    want_mean, want_total = mo.moments_finish(exact)
    cterms = mo.cov_terms(case.pose7, w, mean)
    cexact = mo.exact_sums(cterms)
    cbound = mo.sum_bound(cterms) + mo.cov_budget(case.pose7, w, mean)
    assert mo.wrap_margin(case.pose7, w, mean) > 1e-5
    d_pose, d_w = dev(case.pose7), dev(w)
    if len(cfg[0]) == 1:
        # one context: the single engine's kernels on the same floats
        rec = moments_record(engine, d_pose, d_w, dev(bias), n)
        within("jump bias, one context: ten sums", rec[:10], exact, bound, terms)
        fin = engine.moments_finish(rec)
        np.testing.assert_array_equal(mean, fin[0])
        assert (total, im, ib) == fin[1:]
        np.testing.assert_array_equal(fin[0], mo.moments_finish(rec[:10])[0])
        crec = record(engine, 22, lambda r: engine.covariance_partial_device(d_pose, d_w, n, mean, r))
        within("group covariance, one context: 22 sums", crec, cexact, cbound, cterms)
        np.testing.assert_array_equal(cov, mo.covariance_finish(crec))
    else:
        one_ulp("three contexts: total", total, want_total)
        one_ulp("three contexts: position", mean[:3], want_mean[:3])
        angle = mo.quat_angle(mean[3:], want_mean[3:])
        print("three contexts: rotation %.3g rad" % angle)
        assert angle < 5e-4 and abs(np.linalg.norm(mean[3:].astype(D)) - 1.0) < 1e-6
        want_cov = mo.covariance_finish(cexact)
        pos = np.ix_(range(3), range(3))
        one_ulp("three contexts: position block of the covariance", cov[pos], want_cov[pos])
        # the other entries: the sum's own bound (angle budget included) over sum w, and the float roundings of the quotient
        tol = np.zeros((6, 6), D)
        for i, (j, k) in enumerate(mo.PAIRS):
            tol[j, k] = tol[k, j] = cbound[i] / cexact[21] + float(np.spacing(np.abs(want_cov[j, k])))
        within("three contexts: covariance", cov, want_cov.astype(D), tol)
        np.testing.assert_array_equal(cov, cov.T)


# ---- pf::measure and the update past the cap ------------------------------------------------------------------------------------
def measure_inputs(n, seed):
    rng = np.random.default_rng(seed)
    w0 = rng.uniform(0.2, 1.0, n).astype(F)
    w0[rng.permutation(n)[: n // 10]] = 0.0  # a tenth is dead (skipped by the entropy sum, pf.h:267-270)
    w0 /= w0.sum(dtype=D)
    lik = rng.uniform(1.0, 50.0, n).astype(F)
    beam = rng.uniform(0.2, 1.0, n).astype(F)
    extra = rng.uniform(0.1, 0.4, n).astype(F)
    ratio = rng.uniform(0.2, 0.8, n).astype(F)
    sent = mo.sentinels(n)
    w0[sent] = F(32.0 / n)
    ratio[sent[-1]], ratio[sent[-2]] = 0.9375, 0.0625  # the extreme ratios sit on the last two sentinels
    return w0, lik, beam, extra, ratio


@pytest.mark.parametrize("n", [CAP - 1, CAP, CAP + 1, 2 * CAP + 1])
def test_pf_measure_against_the_exact_sum(engine, n):
    for seed in range(n, n + 16):
        w0, lik, beam, extra, ratio = measure_inputs(n, seed)
        wn = mo.pf_weights(w0, lik, beam, extra)
        want_w, want_ent, s, edge, bound = mo.pf_normalised(wn)
        if edge > bound:  # the device's fp64 sum rounds to the same float
            break
    assert edge > bound, "no seed on which the sum keeps clear of a float rounding boundary"
    for i in mo.sentinels(n):
        assert wn[i] >= 1000.0 * bound  # a lost sentinel moves the sum by a thousand bounds
    print("n %d: sum %.17g, %.3g of its bound away from a rounding boundary" % (n, s, edge / bound))
    got = engine.pf_measure(w0, lik, beam, extra, ratio)
    assert not got["restored"]
    np.testing.assert_array_equal(got["weights"], want_w)
    rel = abs(got["entropy"] - want_ent) / abs(want_ent)
    print("n %d: entropy relative error %.3g" % (n, rel))
    assert rel < 1e-6
    assert got["match_ratio_min"] == 0.0625 and got["match_ratio_max"] == 0.9375


def test_pf_measure_restores_past_the_cap(engine):
    n = CAP + 1
    w0, lik, beam, extra, ratio = measure_inputs(n, 1)
    got = engine.pf_measure(w0, np.zeros(n, F), beam, extra, ratio)
    assert got["restored"] is True
    np.testing.assert_array_equal(got["weights"], w0)
    assert got["match_ratio_min"] == 0.0625 and got["match_ratio_max"] == 0.9375


@pytest.mark.parametrize("n_p,n_s,n_b", [(CAP, 4352, 3), (CAP + 1, 4352, 3)])
def test_update_weights_on_either_side_of_the_tiled_tail_s_limit(engine, n_p, n_s, n_b):
    """Behind the tiled likelihood kernel the update's tail is lik_pf_partial_kernel up to 1024 x 256 particles and
    lik_finalize_kernel + pf_partial_kernel from one more (pf_tiles_fit): the weights of either against the numpy statement over
    the update's own likelihoods and beam scores."""
    from mcl_3dl_amd.synthetic import make_scene
    sc = make_scene(n=91, n_p=n_p, n_s=n_s, n_b=n_b, seed=900 + n_b)
    engine.set_map(sc.map_xyz, sc.map_label, stamp=6800 + n_p % 7, dist_weight=(1.0, 1.0, 5.0))
    engine.set_likelihood_params()
    engine.set_beam_params(num_points=n_b)
    try:
        extra = np.random.default_rng(n_p).uniform(0.1, 0.4, n_p).astype(F)
        w0 = np.random.default_rng(n_s).uniform(0.0, 1.0, n_p).astype(F)
        w0[::7] = 0.0
        w0[mo.sentinels(n_p)] = 32.0
        got = engine.measure_update(sc.poses, w0, sc.scan_lik, sc.scan_beam, sc.scan_beam_label, sc.origins, extra=extra)
    finally:
        engine.set_beam_params()
    assert not got["restored"]
    wn = mo.pf_weights(w0, got["lik"], got["beam"], extra)
    _, want_ent, s, edge, bound = mo.pf_normalised(wn)
    # every float32 an fp64 sum within the bound of the exact one can round to (one, unless the sum sits at a rounding boundary)
    sums = sorted({float(F(s - bound)), float(F(s)), float(F(s + bound))})
    print("n_p %d: %d candidate sum(s), %.3g bounds away from a rounding boundary" % (n_p, len(sums), edge / bound))
    for i in mo.sentinels(n_p):
        assert wn[i] >= 1000.0 * bound
    assert any(np.array_equal(got["weights"], (wn / F(sf)).astype(F)) for sf in sums)
    assert abs(got["entropy"] - want_ent) / abs(want_ent) < 1e-6
    assert got["match_ratio_max"] == float(got["quality"].max()) and got["match_ratio_min"] == float(got["quality"].min())
