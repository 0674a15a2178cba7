"""Wall time per call of resampling the resident particles in ONE call — mcl3dl_hip_group_resample_drawn and
_group_resize_resident (float_prefix.h, resample_prefix_kernels.h) — beside the three-call sequences they stand for, on the same
group: group_resample_begin + rng_uniform + _plan + _apply_drawn, and group_resample_begin(n_out) + _plan(1) + _apply. One GPU;
64, 4096, 65 536 and 262 144 particles with tie-free weights (route 0), 4096 and 262 144 with 10 % dead particles (route 1: the
tie groups are ordered on the host either way), resizeParticle to three quarters at 262 144. Ten calls each after two warm-up
calls: min / median / max. The particles are uploaded again in front of every call, outside the timed part. Then the same loop
where every rank gathers weights, states and odometry noise (host_group_gather.h): one rank through the sharded path over RCCL
and three contexts combined through the host, 4096 and 70 001 particles (profiles/group_gather_once_ab.txt).
  --profile : three calls each of the one-call forms only (the run rocprofv3 --kernel-trace --stats wraps)
  --write   : runs itself both ways and writes profiles/resample_resident.txt (the CPU replay's step counts appended) and
              profiles/resample_resident_kernel_stats.csv"""
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

profile_only = "--profile" in sys.argv
WARM, REPS = (1, 3) if profile_only else (2, 10)
SIGMA6 = np.array([0.1, 0.1, 0.05, 0.01, 0.01, 0.05], np.float32)
SEED = 12345


def times(setup, f):
    ts = []
    for i in range(WARM + REPS):
        setup()
        t = time.perf_counter()
        f()
        if i >= WARM:
            ts.append((time.perf_counter() - t) * 1e3)
    return "min %.4f median %.4f max %.4f ms" % (min(ts), float(np.median(ts)), max(ts))


def main():
    from mcl_3dl_amd import capi
    g = capi.Group([0])

    def three_calls():
        pstep = g.resample_begin()
        ip, st = capi.rng_uniform(SEED, 0.0, pstep)
        g.resample_plan(0, ip)
        g.resample_apply_drawn(SIGMA6, st)

    for n, dead in ((64, 0), (4096, 0), (65536, 0), (262144, 0), (4096, 0.1), (262144, 0.1)):
        rng = np.random.default_rng(n)
        st = rng.normal(0, 1, (n, 13)).astype(np.float32)
        st[:, 3:7] /= np.linalg.norm(st[:, 3:7], axis=1, keepdims=True)
        w = rng.uniform(0.5, 1.5, n)
        if dead:
            w[rng.choice(n, int(dead * n), replace=False)] = 0
        w = (w / w.sum()).astype(np.float32)
        g.upload_state(st, w)
        route = g.resample_drawn(SIGMA6, SEED)[4]
        print("%d particles, %s (route %d)" % (n, "%d %% dead" % (100 * dead) if dead else "tie-free", route))
        print("  resample_drawn (one call)                       : " + times(lambda: g.upload_state(st, w),
                                                                               lambda: g.resample_drawn(SIGMA6, SEED)))
        if not profile_only:
            print("  begin + rng_uniform + plan + apply_drawn         : " + times(lambda: g.upload_state(st, w), three_calls))
        if n == 262144 and not dead:
            n_out = 3 * n // 4

            def resize_three():
                g.resample_begin(n_out)
                g.resample_plan(1)
                g.resample_apply()
            print("  resize_resident to %d (one call)            : " % n_out + times(lambda: g.upload_state(st, w),
                                                                                     lambda: g.resize_resident(n_out)))
            if not profile_only:
                print("  begin(%d) + plan(1) + apply                 : " % n_out + times(lambda: g.upload_state(st, w),
                                                                                         resize_three))
    g.close()
    if not profile_only:
        gathered()


def gathered():
    """The same loop where every rank gathers the weights, the states and the odometry noise: one rank through the sharded path
    (RCCL all-gathers with one rank) and three contexts on the one GPU combined through the host."""
    from mcl_3dl_amd import capi
    for label, devices, collective in (("one rank, direct_single 0 (RCCL)", [0], None), ("three contexts, host gather", [0, 0, 0], "host")):
        g = capi.Group(devices, collective=collective)
        g.set_option("direct_single", 0)

        def three_calls():
            pstep = g.resample_begin()
            ip, st = capi.rng_uniform(SEED, 0.0, pstep)
            g.resample_plan(0, ip)
            g.resample_apply_drawn(SIGMA6, st)

        for n in (4096, 70001):
            rng = np.random.default_rng(n)
            st = rng.normal(0, 1, (n, 13)).astype(np.float32)
            st[:, 3:7] /= np.linalg.norm(st[:, 3:7], axis=1, keepdims=True)
            w = rng.uniform(0.5, 1.5, n)
            w = (w / w.sum()).astype(np.float32)
            noise = rng.normal(0, 0.1, (n, 4)).astype(np.float32)

            def setup():
                g.upload_state(st, w)
                g.set_odom_noise(noise)

            print("%s, %d particles, tie-free, odometry noise installed" % (label, n))
            print("  resample_drawn (one call)                       : " + times(setup, lambda: g.resample_drawn(SIGMA6, SEED)))
            print("  begin + rng_uniform + plan + apply_drawn         : " + times(setup, three_calls))
            print("  resize_resident to %d (one call)              : " % (3 * n // 4) + times(setup, lambda: g.resize_resident(3 * n // 4)))
        g.close()


def write():
    prof = os.path.join(ROOT, "profiles")
    me = os.path.abspath(__file__)
    out = subprocess.run([sys.executable, me], check=True, capture_output=True, text=True, timeout=900).stdout
    d = tempfile.mkdtemp(prefix="resample_resident_prof_")
    try:
        emul = os.path.join(d, "float_prefix_emul.bin")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", emul, os.path.join(ROOT, "tests", "cpp", "float_prefix_emul.cpp")],
                       check=True)
        steps = subprocess.run([emul, "selftest"], check=True, capture_output=True, text=True, timeout=600).stdout
        with open(os.path.join(prof, "resample_resident.txt"), "w") as f:
            f.write(out)
            f.write("\nfloat_prefix.h replayed on the CPU (tests/cpp/float_prefix_emul.cpp): steps behind the 256-term head\n")
            f.write(steps)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me,
                        "--profile"], check=True, timeout=900, stdout=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        shutil.copy(stats[0], os.path.join(prof, "resample_resident_kernel_stats.csv"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(out)


if __name__ == "__main__":
    write() if "--write" in sys.argv else main()
