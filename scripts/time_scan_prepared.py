"""Wall time per scan of the prepared route on a device group — mcl3dl_hip_group_scan_finish_drawn +
mcl3dl_hip_group_update_resident_prepared (api_group_state.inl, rng_index_kernels.h) — beside the long way round through the entry
points that existed before them: mcl3dl_hip_scan_finish with host-drawn indices (drawn outside the timed region), two
mcl3dl_hip_scan_download calls and mcl3dl_hip_group_update_resident with the host scans. One GPU; 4096 particles x (96 + 3) and
x (16 384 + 512) points; ten calls each after two warm-up calls: min / median / max. Each call is synchronous.
  --profile : three calls each and no long way round (the run rocprofv3 --kernel-trace --stats wraps)
  --write   : runs itself both ways and writes profiles/scan_prepared.txt and profiles/scan_prepared_kernel_stats.csv"""
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
LEAF = (0.05, 0.05, 0.05)
CLIP_LIK = (0.5, 10.0, -2.0, 2.0)
CLIP_BEAM = (0.5, 4.0, -2.0, 2.0)
SEED = 12345
N_P = 4096


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
    from mcl_3dl_amd.synthetic import make_scene
    import rng_index_ref as rir
    sc = make_scene(n=91, n_p=300, n_s=20000, n_b=2000, seed=43)
    cloud = np.concatenate([sc.scan_lik, sc.scan_beam], 0)
    g = capi.Group([0])
    g.set_map(sc.map_xyz, sc.map_label, stamp=1, dist_weight=(1.0, 1.0, 3.0))
    g.set_likelihood_params()
    g.set_beam_params(num_points=512)
    reps = (N_P + len(sc.poses) - 1) // len(sc.poses)
    s = np.zeros((N_P, 13), np.float32)
    s[:, :7] = np.tile(sc.poses, (reps, 1))[:N_P]
    g.upload_state(s, np.full(N_P, 1.0 / N_P, np.float32))
    ctx = g.context(0)
    _, n_lik, n_beam = g.scan_begin(cloud, None, leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)
    print("cloud %d points, clipped %d / %d, %d particles" % (len(cloud), n_lik, n_beam, N_P))
    for n_s, n_b in ((96, 3), (16384, 512)):
        idx_l, idx_b, _ = rir.scan_draws(SEED, n_s, n_lik, n_b, n_beam)
        print("%d + %d points" % (n_s, n_b))

        def drawn():
            g.scan_finish_drawn(n_s, n_b, sc.origins, SEED)

        def prepared():
            g.update_resident_prepared(fetch=False)

        def new_route():
            drawn()
            prepared()
        print("  group_scan_finish_drawn                         : " + times(drawn))
        print("  update_resident_prepared                        : " + times(prepared))
        print("  both (the prepared route)                       : " + times(new_route))
        if profile_only:
            continue

        def finish():
            ctx.scan_finish(idx_l, idx_b, origins=sc.origins)

        def long_way():
            finish()
            lik_xyz, _ = ctx.scan_download(3)
            beam_xyz, beam_label = ctx.scan_download(4)
            g.update_resident(lik_xyz, beam_xyz, beam_label, sc.origins, fetch=False)
        print("  scan_finish (indices drawn beforehand)          : " + times(finish))
        print("  scan_finish + 2 downloads + update_resident     : " + times(long_way))
    g.close()


def write():
    prof = os.path.join(ROOT, "profiles")
    me = os.path.abspath(__file__)
    out = subprocess.run([sys.executable, me], check=True, capture_output=True, text=True, timeout=900).stdout
    with open(os.path.join(prof, "scan_prepared.txt"), "w") as f:
        f.write(out)
    d = tempfile.mkdtemp(prefix="scan_prepared_prof_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me,
                        "--profile"], check=True, timeout=900, stdout=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        shutil.copy(stats[0], os.path.join(prof, "scan_prepared_kernel_stats.csv"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(out)


if __name__ == "__main__":
    write() if "--write" in sys.argv else main()
