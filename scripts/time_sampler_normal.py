"""mcl3dl_hip_scan_normal_weights on clipped clouds of about 4 000 and about 65 536 points: host wall time
per call over ten calls after a warm-up. Run it under rocprofv3 --kernel-trace --stats for the kernel times.
`--neighbours` also prints the mean neighbour count of each cloud from the numpy oracle (slow, not timed)."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mcl_3dl_amd import capi  # noqa: E402
from mcl_3dl_amd.synthetic import make_config  # noqa: E402

R, FPC, MAX_WEIGHT = 0.4, np.array([0.8, 0.6, 0.0], np.float32), 5.0
sc = make_config("C3", seed=12345)
rng = np.random.default_rng(4)
big = np.concatenate([sc.scan_lik + rng.normal(0, 0.02, sc.scan_lik.shape).astype(np.float32) for _ in range(4)], 0)[:65536]
clouds = [("4k", np.ascontiguousarray(big[:4096], np.float32)), ("64k", np.ascontiguousarray(big, np.float32))]
eng = capi.Engine(0)
cl, cb = (0.5, 10.0, -2.0, 2.0), (0.5, 4.0, -2.0, 2.0)
N, WARM = 10, 3
for name, raw in clouds:
    n_full, n_lik, n_beam = eng.scan_begin(raw, None, leaf=None, clip_lik=cl, clip_beam=cb)
    for with_normals in (False, True):
        t = []
        for it in range(N + WARM):
            t0 = time.perf_counter()
            cum, nrm, n_without = eng.scan_normal_weights(1, R, FPC, MAX_WEIGHT, normals=with_normals)
            t.append(time.perf_counter() - t0)
        t = np.array(t[WARM:]) * 1e3
        print("%s: %d points in, %d in the clipped likelihood cloud, normals %s: %.3f ms per call (min %.3f, max %.3f), "
              "%d without a normal, cum[-1] = %.6f" % (name, len(raw), n_lik, "downloaded" if with_normals else "not asked for",
                                                       t.mean(), t.min(), t.max(), n_without, cum[-1]))
    if "--neighbours" in sys.argv:
        sys.path.insert(0, "tests")
        import sampler_normal_ref as snr  # noqa: E402
        cloud, _ = eng.scan_download(1)
        cnt = snr.oracle(cloud, R)["count"]
        print("%s: neighbours per point: mean %.1f, max %d" % (name, cnt.mean(), cnt.max()))
