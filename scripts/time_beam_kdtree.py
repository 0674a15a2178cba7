"""The beam model with the kd-tree caster (mcl3dl_hip_set_beam_raycast 1 = RaycastUsingKDTree, the reference's default) against
the DDA caster (mode 0) on the same build and the same scene, and against the oracle's kd-tree caster on one CPU thread:
bench config C3's map (hollow cube n = 408: 998 784 points), dist_weight (1, 1, 5), at the reference's operating shape
(4096 particles x 3 rays) and at C3's beam shape (4096 x 512). The beam model alone (mcl3dl_hip_measure_device without the
likelihood outputs): hipEvent time of the beam kernel group, and wall time per call ending in a synchronise.
  --profile : few repetitions and no oracle (the run rocprofv3 --kernel-trace --stats wraps)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import make_config
DW = (1.0, 1.0, 5.0)
KERNEL_BEAM = 1
profile_only = "--profile" in sys.argv
WARM, REPS = (2, 5) if profile_only else (10, 50)
dev = torch.device("cuda", 0)
for n_p, n_b, n_oracle in ((4096, 3, 4096), (4096, 512, 32)):
    sc = make_config("C3", n_p=n_p, n_s=16, n_b=n_b, seed=12345)
    eng = capi.Engine(0)
    eng.set_map(sc.map_xyz, sc.map_label, stamp=1, dist_weight=DW)
    eng.set_likelihood_params()
    eng.set_beam_params(num_points=n_b)
    eng.upload_scan(None, sc.scan_beam, sc.scan_beam_label, sc.origins)
    d_pose = torch.from_numpy(np.ascontiguousarray(sc.poses)).to(dev)
    d_beam = torch.empty(n_p, device=dev)
    torch.cuda.synchronize()
    print("shape %d particles x %d rays = %d rays, map %d points" % (n_p, n_b, n_p * n_b, len(sc.map_xyz)))
    scores = {}
    for mode, name in ((0, "mode 0 RaycastUsingDDA   "), (1, "mode 1 RaycastUsingKDTree")):
        eng.set_beam_raycast(mode)
        t = time.perf_counter()
        eng.measure_device(d_pose, n_p, None, None, d_beam); eng.synchronize()
        first = (time.perf_counter() - t) * 1e3
        for _ in range(WARM):
            eng.measure_device(d_pose, n_p, None, None, d_beam)
        eng.synchronize()
        wall = []
        for _ in range(REPS):
            t = time.perf_counter()
            eng.measure_device(d_pose, n_p, None, None, d_beam); eng.synchronize()
            wall.append((time.perf_counter() - t) * 1e3)
        eng.set_kernel_timing(True); eng.reset_kernel_time()
        for _ in range(REPS):
            eng.measure_device(d_pose, n_p, None, None, d_beam)
        eng.synchronize()
        ms, launches = eng.kernel_time(KERNEL_BEAM)
        eng.set_kernel_timing(False)
        scores[mode] = d_beam.cpu().numpy().copy()
        print("  %s: beam kernel group %.4f ms per call (hipEvents, %d calls); wall per call min %.4f median %.4f max %.4f ms; "
              "first call %.2f ms (builds the caster's map structures)"
              % (name, ms / max(launches, 1), launches, min(wall), float(np.median(wall)), max(wall), first))
    print("  particles whose score differs between the casters: %d of %d" % (int(np.sum(scores[0] != scores[1])), n_p))
    if not profile_only:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from oracle import pyoracle
        kind = "ref" if pyoracle.available("ref") else "port"
        o = pyoracle.Oracle(kind, 20.0, 0.4)
        o.set_map(sc.map_xyz, sc.map_label, dist_weight=DW)
        o.set_beam_params(pyoracle.BeamParams(num_points=n_b, use_raycast_using_dda=False))
        o.beam_measure(sc.poses[:4], sc.scan_beam, sc.scan_beam_label, sc.origins, threads=1)
        want, _, dt = o.beam_measure(sc.poses[:n_oracle], sc.scan_beam, sc.scan_beam_label, sc.origins, threads=1, return_time=True)
        assert np.array_equal(scores[1][:n_oracle], want), "mode 1 differs from the oracle"
        per_ray_us = dt * 1e6 / (n_oracle * n_b)
        print("  %s oracle, RaycastUsingKDTree, ONE thread: %d particles in %.1f ms = %.2f us per ray -> %.1f ms for the whole shape%s; "
              "scores equal mode 1's bit for bit"
              % (kind, n_oracle, dt * 1e3, per_ray_us, per_ray_us * n_p * n_b * 1e-3, "" if n_oracle == n_p else " (scaled from the sample)"))
    eng.close()
