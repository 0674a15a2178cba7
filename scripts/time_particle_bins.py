"""Wall time per call of mcl3dl_hip_group_particle_bins (particle_bins_kernels.h) on a group of one device,
beside what a caller has without it: group_download_state plus a host count of the distinct keys (np.unique over the same
keys, tests/particle_bins_ref.py). 4096, 65 536 and 450 408 resident particles (the last: the project's own global-localisation
figure), two distributions each:
  spread     laid out as global localisation seeds them — one particle per (lattice point, rotation of div_yaw = 8), bins of the
             lattice's edge and 8 sectors: nearly every bin holds one particle
  converged  everything within a few centimetres and degrees of one pose: at most 8 bins
Ten calls each after two warm-up calls: min / median / max. The one thing to read off: the converged case is not slower than
the spread one by more than the sort's own difference — the segmented reduction's cost does not depend on the distribution.
  --profile : three calls each of particle_bins only (the run rocprofv3 --kernel-trace --stats wraps)
  --write   : runs itself both ways and writes profiles/particle_bins.txt (the new kernels' and the sort's rows of the kernel
              statistics appended)"""
import csv
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
DIV_YAW, GRID = 8, 0.3
SIZES = (4096, 65536, 450408)


def times(f):
    ts = []
    for i in range(WARM + REPS):
        t = time.perf_counter()
        f()
        if i >= WARM:
            ts.append((time.perf_counter() - t) * 1e3)
    return "min %.4f median %.4f max %.4f ms" % (min(ts), float(np.median(ts)), max(ts))


def spread(n, capi):
    """n = points x DIV_YAW particles, particle i = point i / DIV_YAW with rotation i % DIV_YAW (cbGlobalLocalization's layout)."""
    rng = np.random.default_rng(n)
    n_points = n // DIV_YAW
    side = int(np.ceil(np.sqrt(n_points / 2.0)))
    cells = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(2), indexing="ij"), -1).reshape(-1, 3)[:n_points]
    points = ((cells + rng.uniform(0.1, 0.9, cells.shape)) * GRID).astype(np.float32)
    rot = capi.global_localization_rotations(DIV_YAW)
    # the rotations sit ON the sector boundaries (2 pi j / 8): half a sector further they are clear of them
    half = np.float32(np.pi / DIV_YAW / 2)
    turn = np.array([0, 0, np.sin(half), np.cos(half)], np.float32)
    rot = np.stack([quat_mul(q, turn) for q in rot]).astype(np.float32)
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = np.repeat(points, DIV_YAW, axis=0)
    s[:, 3:7] = np.tile(rot, (n_points, 1))
    return s, np.full(n, np.float32(1.0 / n_points))


def quat_mul(a, b):
    ax, ay, az, aw = (float(v) for v in a)
    bx, by, bz, bw = (float(v) for v in b)
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def converged(n):
    rng = np.random.default_rng(n + 1)
    s = np.zeros((n, 13), np.float32)
    s[:, :3] = np.array([3.1, 4.2, 0.4]) + rng.normal(0, 0.02, (n, 3))
    yaw = 0.3 + rng.normal(0, 0.02, n)
    s[:, 5], s[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    w = rng.uniform(0.5, 1.5, n)
    return s, (w / w.sum()).astype(np.float32)


def main():
    import particle_bins_ref as ref
    from mcl_3dl_amd import capi
    bin3 = (GRID, GRID, GRID)
    table = capi.yaw_sector_table(DIV_YAW)
    g = capi.Group([0])

    def host_count():
        s, _ = g.download_state()
        grid = ref.make_grid(s[:, :3], bin3, DIV_YAW)
        return len(np.unique(ref.keys(s[:, :7], grid, table)))

    for n in SIZES:
        n -= n % DIV_YAW
        for label, (s, w) in (("spread", spread(n, capi)), ("converged", converged(n))):
            g.upload_state(s, w)
            got = g.particle_bins(bin3, yaw_bins=DIV_YAW, top_k=0)
            if not profile_only:
                assert got["occupied"] == host_count(), (got["occupied"], host_count())
            print("%d particles, %s: %d occupied bins (KLD bound at epsilon 0.05, z 2.326: %d)"
                  % (n, label, got["occupied"], capi.kld_bound(got["occupied"], 0.05, 2.326)))
            print("  particle_bins, top_k 0                          : " + times(lambda: g.particle_bins(bin3, DIV_YAW, 0)))
            print("  particle_bins, top_k 16                         : " + times(lambda: g.particle_bins(bin3, DIV_YAW, 16)))
            if not profile_only:
                print("  download_state alone                            : " + times(g.download_state))
                print("  download_state + host keys + np.unique          : " + times(host_count))
    g.close()


def write():
    prof = os.path.join(ROOT, "profiles")
    me = os.path.abspath(__file__)
    out = subprocess.run([sys.executable, me], check=True, capture_output=True, text=True, timeout=900).stdout
    d = tempfile.mkdtemp(prefix="particle_bins_prof_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me,
                        "--profile"], check=True, timeout=900, stdout=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(stats[0])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    with open(os.path.join(prof, "particle_bins.txt"), "w") as f:
        f.write(out)
        f.write("\nrocprofv3 --kernel-trace --stats over `--profile` (a run of its own: the six cases above, four calls of each top_k "
                "each; times in ns)\n")
        f.write("%-64s %8s %14s %12s %12s %12s\n" % ("kernel", "calls", "total", "average", "min", "max"))
        for r in rows:
            name = r.get("Name", "")
            if any(k in name for k in ("pb_", "rs_", "radix", "sort", "rocprim")):
                f.write("%-64s %8s %14s %12s %12s %12s\n" % (name[:64], r.get("Calls"), r.get("TotalDurationNs"),
                                                           r.get("AverageNs"), r.get("MinNs"), r.get("MaxNs")))
    print(open(os.path.join(prof, "particle_bins.txt")).read())


if __name__ == "__main__":
    write() if "--write" in sys.argv else main()
