"""Per-call times of the between-scan calls on resident particles (api_group_motion.inl) — predict, measure_imu,
set_odom_noise, add_noise — at 4096, 65 536 and 262 144 particles on one GPU, beside the download_state + upload_state round
trip a caller needs without them (+ set_odom_noise again, since an upload zeroes the noise). Each call is synchronous (it returns after its stream is idle): median of 50 calls after 5
warm-up calls. Run on the GPU box; prints one JSON line per size."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mcl_3dl_amd import capi  # noqa: E402


def timeit(f, n=50):
    for _ in range(5):
        f()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 65536, 262144]
    rng = np.random.default_rng(1)
    prev = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
    cur = np.array([0.1, 0.01, 0, 0, 0, 0.0499792, 0.9987503], np.float32)
    acc = np.array([0.1, -0.1, 9.8], np.float32)
    g = capi.Group([0])
    for n in sizes:
        st = np.zeros((n, 13), np.float32)
        st[:, :3] = rng.uniform(-3, 3, (n, 3))
        q = rng.normal(0, 0.1, (n, 4))
        q[:, 3] += 1
        st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        nz4 = (rng.normal(0, 0.05, (n, 4))).astype(np.float32)
        nz13 = np.zeros((n, 13), np.float32)
        nz13[:, 6] = 1.0
        w = np.full(n, 1.0 / n, np.float32)
        g.upload_state(st, w)
        g.set_odom_noise(nz4)

        def round_trip():
            s, ww = g.download_state()
            g.upload_state(s, ww)
            g.set_odom_noise(nz4)
        r = dict(n=n,
                 predict_ms=timeit(lambda: g.predict(prev, cur, 0.1)),
                 measure_imu_ms=timeit(lambda: g.measure_imu(acc, 0.3, fetch=False)),
                 set_odom_noise_ms=timeit(lambda: g.set_odom_noise(nz4)),
                 add_noise_ms=timeit(lambda: g.add_noise(nz13)),
                 download_upload_round_trip_ms=timeit(round_trip))
        print(json.dumps(r), flush=True)
    g.close()


if __name__ == "__main__":
    main()
