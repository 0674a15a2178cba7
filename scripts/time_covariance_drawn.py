"""mcl3dl_hip_group_covariance_drawn against the long way round, one device, world 1: host wall time per call over
ten calls after a warm-up, at n = 46 341 and 450 408 resident particles with ratio 0.1 and at 450 408 with the node's own ratio
for num_particles = 64, max(0.1f, 64.f / n).

  drawn      group_covariance_drawn: the shuffle on the device (doubtful attempts, resolve, targets, sort, chain walks), the windowed
             covariance over its first m entries, one call
  long way   std::iota + std::shuffle of n size_t on one core, timed INSIDE tests/cpp/rng_shuffle_emul.cpp (g++ -O2, `time`), plus
             group_covariance_sampled with the m indices (validated and uploaded by the call)
  prefix     rng_shuffle_prefix alone with m = n / 10 (the indices come home), for what the shuffle costs without the reduction
Run it under rocprofv3 --kernel-trace --stats for the kernel times (shuffle_doubt_count / _emit / resolve / targets / chain kernels,
rs_* of the sort, pf_covariance_window_kernel)."""
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import rng_shuffle_ref as rsr  # noqa: E402
from mcl_3dl_amd import capi  # noqa: E402

N, WARM, STATE = 10, 3, 1
F = np.float32
exe = rsr.emul_exe()  # compiled before anything is timed


def timed(f):
    t = []
    for _ in range(N + WARM):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return np.array(t[WARM:]) * 1e3


def particles(n):
    rng = np.random.default_rng(n)
    s = np.zeros((n, 13), F)
    s[:, :3] = rng.normal(0, 0.5, (n, 3))
    q = rng.normal(0, 0.05, (n, 4))
    q[:, 3] += 1.0
    s[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    w = rng.uniform(0.2, 1.0, n)
    return s, (w / w.sum()).astype(F)


g = capi.Group([0])
eng = capi.Engine(0)
mean7 = np.array([0, 0, 0, 0, 0, 0, 1], F)
for n, ratio, what in ((46341, 0.1, "ratio 0.1"), (450408, 0.1, "ratio 0.1"),
                       (450408, float(max(F(0.1), F(64) / F(450408))), "the node's ratio for num_particles = 64")):
    s, w = particles(n)
    g.upload_state(s, w)
    m = rsr.sample_count(n, ratio)
    whole, behind, fields = rsr.emul("device", STATE, n, m)
    cov, n_sampled, st = g.covariance_drawn(mean7, ratio, STATE)
    assert (n_sampled, st) == (m, behind)
    assert np.array_equal(cov, g.covariance_sampled(mean7, whole))
    t_host = float(subprocess.run([exe, "time", str(STATE), str(n), "20"], check=True, capture_output=True,
                                  text=True).stdout.split()[0].split("=")[1])
    t_new = timed(lambda: g.covariance_drawn(mean7, ratio, STATE))
    t_old = timed(lambda: g.covariance_sampled(mean7, whole))
    t_pre = timed(lambda: eng.rng_shuffle_prefix(n, m, STATE))
    t_all = timed(lambda: g.covariance(mean7))
    print("n %d, %s (m = %d; %d doubtful, %d rejected attempts): drawn %.3f ms per call (min %.3f, max %.3f); long way round "
          "%.3f ms = std::shuffle on one core %.3f ms + covariance_sampled with its upload %.3f ms (min %.3f, max %.3f); "
          "rng_shuffle_prefix alone %.3f ms (min %.3f); group_covariance over all n %.3f ms; matrices equal"
          % (n, what, m, fields["doubtful"], fields["rejected"], t_new.mean(), t_new.min(), t_new.max(), t_host + t_old.mean(),
             t_host, t_old.mean(), t_old.min(), t_old.max(), t_pre.mean(), t_pre.min(), t_all.mean()))
g.close()
eng.close()
