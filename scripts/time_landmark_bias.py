"""Wall time per call of the two pose-reading calls on resident particles — mcl3dl_hip_group_expectation_jump_bias and
mcl3dl_hip_group_measure_landmark (api_group_state.inl, api_group_motion.inl, landmark_kernels.h) — beside the long way round
through the entry points that existed before them: download_state + expectation(bias = host array) (the numpy bias itself not
counted), and download_state + upload_state (what a landmark update weighed on the CPU moves). One GPU, 4096 and 262 144
particles, ten calls each after two warm-up calls: min ... max. Each call is synchronous.
  --profile : three calls each and no long way round (the run rocprofv3 --kernel-trace --stats wraps)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mcl_3dl_amd import capi  # noqa: E402

profile_only = "--profile" in sys.argv
WARM, REPS = (1, 3) if profile_only else (2, 10)


def times(f):
    for _ in range(WARM):
        f()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return "min %.4f median %.4f max %.4f ms" % (min(ts), float(np.median(ts)), max(ts))


def main():
    rng = np.random.default_rng(1)
    prev = np.array([0.1, -0.2, 0.0, 0, 0, 0.0499792, 0.9987503], np.float32)
    m7 = np.array([0.3, 0.1, 0.0, 0, 0, 0, 1], np.float32)
    cov = np.diag([9.0, 9.0, 9.0, 1.0, 1.0, 1.0])
    g = capi.Group([0])
    for n in (4096, 262144):
        st = np.zeros((n, 13), np.float32)
        st[:, :3] = rng.uniform(-3, 3, (n, 3))
        q = rng.normal(0, 0.2, (n, 4))
        q[:, 3] += 1
        st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        host_bias = np.full(n, 0.5, np.float32)
        g.upload_state(st)
        print("%d particles" % n)
        print("  expectation_jump_bias                      : " + times(lambda: g.expectation_jump_bias(prev, 2.0, 1.57)))
        print("  expectation_jump_bias, biases fetched      : "
              + times(lambda: g.expectation_jump_bias(prev, 2.0, 1.57, fetch_bias=True)))
        print("  expectation(bias = NULL)                   : " + times(lambda: g.expectation()))
        print("  measure_landmark(fetch=False)              : " + times(lambda: g.measure_landmark(m7, cov, fetch=False)))
        print("  download_particle                          : " + times(lambda: g.download_particle(n // 2)))
        if profile_only:
            continue

        def bias_long_way():
            g.download_state()
            g.expectation(bias=host_bias)

        def round_trip():
            s, w = g.download_state()
            g.upload_state(s, w)
        print("  download_state + expectation(bias = array) : " + times(bias_long_way))
        print("  download_state + upload_state              : " + times(round_trip))
    g.close()


if __name__ == "__main__":
    main()
