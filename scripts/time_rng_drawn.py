"""Wall time per call of the four entry points that draw the filter's noise on the device — mcl3dl_hip_group_add_noise_drawn,
_init_drawn, _draw_odom_noise, _resample_apply_drawn (api_rng.inl, rng_kernels.h) — beside the long way round through the entry
points that existed before them: the same draws made on the host (the reference's generateNoise loop through oracle/_ref where it
is built, the standard library's stream through tests/cpp/rng_polar_emul.cpp otherwise; the odometry stream always the latter),
uploaded and handed to add_noise / upload_state / set_odom_noise / resample_apply. One GPU; 4096, 65 536 and 450 408 particles;
ten calls each after two warm-up calls: min / median / max. Each call is synchronous.
  --profile : three calls each and no long way round (the run rocprofv3 --kernel-trace --stats wraps)
  --write   : runs itself both ways and writes profiles/rng_drawn.txt and profiles/rng_drawn_kernel_stats.csv"""
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

profile_only = "--profile" in sys.argv
WARM, REPS = (1, 3) if profile_only else (2, 10)
SIGMA6 = np.array([0.1, 0.1, 0.05, 0.01, 0.01, 0.05], np.float32)
ZERO6 = np.zeros(6, np.float32)
ERR4 = np.array([0.2, 0.05, 0.1, 0.3], np.float32)
MEAN7 = np.array([1.0, -2.0, 0.3, 0, 0, 0.0499792, 0.9987503], np.float32)
SEED = 12345


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
    from mcl_3dl_amd import capi
    import rng_ref
    from oracle import pyoracle
    orc = pyoracle.Oracle("ref") if pyoracle.available("ref") else None
    print("host draws: %s" % ("oracle/_ref (the reference's generateNoise)" if orc else "std::normal_distribution, CPU program"))

    def host_rows(n):
        if orc:
            return orc.resample_draws(SEED, 1.0, SIGMA6, n)[1]
        return rng_ref.noise_rows(rng_ref.stream("std", "fresh", SEED, 6 * n)[0], ZERO6, SIGMA6, n)[0]

    rng = np.random.default_rng(1)
    g = capi.Group([0])
    for n in (4096, 65536, 450408):
        st = rng.normal(0, 1, (n, 13)).astype(np.float32)
        st[:, 3:7] /= np.linalg.norm(st[:, 3:7], axis=1, keepdims=True)
        w = (rng.uniform(0, 1, n) ** 3).astype(np.float32)
        w /= w.sum(dtype=np.float64)
        g.upload_state(st, w)
        print("%d particles" % n)
        print("  add_noise_drawn                            : " + times(lambda: g.add_noise_drawn(SIGMA6, SEED)))
        print("  draw_odom_noise                            : " + times(lambda: g.draw_odom_noise(ERR4, SEED)))
        print("  init_drawn                                 : " + times(lambda: g.init_drawn(MEAN7, SIGMA6, n, SEED)))

        def plan():
            g.upload_state(st, w)
            pstep = g.resample_begin()
            return g.resample_plan(0, 0.5 * pstep)[2]

        def resample_drawn():
            plan()
            g.resample_apply_drawn(SIGMA6, SEED)
        print("  upload + begin + plan (both resample rows)  : " + times(plan))
        print("  upload + begin + plan + resample_apply_drawn: " + times(resample_drawn))
        if profile_only:
            continue

        def noise_long_way():
            g.add_noise(host_rows(n))

        def odom_long_way():
            z = rng_ref.stream("std", "shared", SEED, 4 * n)[0].reshape(n, 4)
            g.set_odom_noise(z[:, [0, 1, 3, 2]] * ERR4[[0, 1, 3, 2]])

        def init_long_way():
            g.upload_state(host_rows(n))

        def resample_long_way():
            g.resample_apply(host_rows(plan()))
        print("  host draw + add_noise                      : " + times(noise_long_way))
        print("  host stream + set_odom_noise               : " + times(odom_long_way))
        print("  host draw + upload_state                   : " + times(init_long_way))
        print("  upload + begin + plan + host draw + apply   : " + times(resample_long_way))
    g.close()


def write():
    prof = os.path.join(ROOT, "profiles")
    me = os.path.abspath(__file__)
    out = subprocess.run([sys.executable, me], check=True, capture_output=True, text=True, timeout=900).stdout
    with open(os.path.join(prof, "rng_drawn.txt"), "w") as f:
        f.write(out)
    d = tempfile.mkdtemp(prefix="rng_drawn_prof_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me,
                        "--profile"], check=True, timeout=900, stdout=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        shutil.copy(stats[0], os.path.join(prof, "rng_drawn_kernel_stats.csv"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(out)


if __name__ == "__main__":
    write() if "--write" in sys.argv else main()
