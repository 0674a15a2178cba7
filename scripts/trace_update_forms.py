"""Calls every host entry point that runs pf::measure or the host-buffer update once per form, at small shapes, and prints one
line per call. Meant to run under a kernel trace on two builds of the library (MCL3DL_HIP_LIB selects the build):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/trace_update_forms.py

The two lists of (kernel name, grid, work-group size), in launch order, can then be compared line by line: the calls below
are deterministic (fixed seeds, one thread per context except the group's workers, which each own a stream)."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcl_3dl_amd import capi  # noqa: E402
from mcl_3dl_amd.synthetic import make_scene  # noqa: E402

N_P = (64, 600, 1100, 4100)
N_S = (96, 4352)
N_B = (0, 3)
DEFAULTS = dict(update_small=1, pf_fused=1, strict_order=2, update_stage=1, update_zero_copy=1)


def scans(sc, n_s, n_b):
    if n_b == 0:
        return sc.scan_lik[:n_s], None, None, None
    return sc.scan_lik[:n_s], sc.scan_beam[:n_b], sc.scan_beam_label[:n_b], sc.origins


def configure(obj, sc):
    obj.set_map(sc.map_xyz, sc.map_label, stamp=1, dist_weight=(1.0, 1.0, 1.0))
    obj.set_likelihood_params()
    obj.set_beam_params(num_points=3)


def states13(sc, n):
    s = np.zeros((n, 13), np.float32)
    s[:, :7] = sc.poses[:n]
    return s


def main():
    sc = make_scene(n=91, n_p=max(N_P), n_s=max(N_S), n_b=max(N_B), seed=5)
    calls = 0

    def say(what, **kw):
        nonlocal calls
        calls += 1
        print(what, " ".join("%s=%s" % kv for kv in kw.items()), flush=True)

    def options(obj, **kw):
        for name, value in dict(DEFAULTS, **kw).items():
            obj.set_option(name, value)

    eng = capi.Engine(0)
    configure(eng, sc)
    # ---- the host-buffer update: every pf::measure form behind both models
    for n_p, n_s, n_b, small, fused, strict in itertools.product(N_P, N_S, N_B, (0, 1), (0, 1), (1, 2)):
        options(eng, update_small=small, pf_fused=fused, strict_order=strict)
        eng.measure_update(sc.poses[:n_p], sc.weights[:n_p], *scans(sc, n_s, n_b))
        say("measure_update", n_p=n_p, n_s=n_s, n_b=n_b, update_small=small, pf_fused=fused, strict_order=strict)
    # ---- ... staged or not, zero-copy or not, into pageable and page-locked arrays
    for n_p, n_b, stage, zero_copy, pinned in itertools.product(N_P, N_B, (0, 1), (0, 1), (0, 1)):
        options(eng, update_stage=stage, update_zero_copy=zero_copy)
        make = eng.host_array if pinned else (lambda n: np.zeros(n, np.float32))
        w, lik, ratio, beam = make(n_p), make(n_p), make(n_p), make(n_p)
        w[:] = sc.weights[:n_p]
        sl, sb, so, og = (None if a is None else np.ascontiguousarray(a) for a in scans(sc, N_S[0], n_b))
        eng.measure_update_into(np.ascontiguousarray(sc.poses[:n_p]), w, sl, sb, so, og, lik, ratio, beam)
        say("measure_update_into", n_p=n_p, n_b=n_b, update_stage=stage, update_zero_copy=zero_copy, page_locked=pinned)
        if pinned:
            for a in (w, lik, ratio, beam):
                eng.host_free(a)
    # ---- the two models only: whole, and in slices
    for n_p, n_s, n_b, stage, zero_copy in itertools.product(N_P, N_S, N_B, (0, 1), (0, 1)):
        options(eng, update_stage=stage, update_zero_copy=zero_copy)
        eng.measure_batch(sc.poses[:n_p], *scans(sc, n_s, n_b))
        say("measure_batch", n_p=n_p, n_s=n_s, n_b=n_b, update_stage=stage, update_zero_copy=zero_copy)
    for n_s, n_b, stage, zero_copy in itertools.product(N_S, N_B, (0, 1), (0, 1)):
        options(eng, update_stage=stage, update_zero_copy=zero_copy)
        eng.measure_batch_begin(sc.poses[:4100], *scans(sc, n_s, n_b), slice_particles=1024)
        eng.measure_batch_wait(4099)
        eng.measure_batch_end()
        say("measure_batch_begin", n_p=4100, n_s=n_s, n_b=n_b, slice_particles=1024, update_stage=stage, update_zero_copy=zero_copy)
    # ---- pf::measure alone
    rng = np.random.default_rng(6)
    for n_p, fused, strict in itertools.product(N_P, (0, 1), (1, 2)):
        options(eng, pf_fused=fused, strict_order=strict)
        lik = rng.uniform(0.1, 1.0, n_p).astype(np.float32)
        eng.pf_measure(sc.weights[:n_p], lik, beam=lik, extra=lik, match_ratio=lik)
        say("pf_measure", n_p=n_p, pf_fused=fused, strict_order=strict)
    eng.close()
    # ---- device groups: one device called directly, one device through the sharded path, two contexts on one device through the host
    acc = np.array([0.3, -0.2, 9.7], np.float32)
    cov = np.diag([0.1, 0.1, 0.1, 0.05, 0.05, 0.05])
    for devices, collective, direct in (((0,), None, 1), ((0,), "host", 0), ((0, 0), "host", 1)):
        g = capi.Group(list(devices), collective=collective)
        g.set_option("direct_single", direct)
        configure(g, sc)
        for n_p, fused, strict in itertools.product(N_P, (0, 1), (1, 2)):
            options(g, pf_fused=fused, strict_order=strict)
            for n_s, n_b in itertools.product(N_S, N_B):
                g.measure_update(sc.poses[:n_p], sc.weights[:n_p], *scans(sc, n_s, n_b))
                g.upload_state(states13(sc, n_p), sc.weights[:n_p])
                g.update_resident(*scans(sc, n_s, n_b))
            g.upload_state(states13(sc, n_p), sc.weights[:n_p])
            g.measure_imu(acc, 0.5)
            g.measure_landmark(sc.poses[0], cov)
            say("group", devices=len(devices), direct_single=direct, n_p=n_p, pf_fused=fused, strict_order=strict)
        g.close()
    print("calls: %d" % calls)


if __name__ == "__main__":
    main()
