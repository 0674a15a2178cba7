"""Wall time per call of mcl3dl_hip_group_init_drawn_multivariate (api_rng.inl, rng_kernels.h: rng_multivariate_state_kernel) — the
`initialpose` particles drawn on the device — at 4096, 65 536 and 450 408 particles on one GPU, beside
  mcl3dl_hip_group_upload_state of as many host rows: the part of the older route that is a call of this library (the host's
      6 n_p normal draws, on one core, come on top of it and are not in the figure), and
  mcl3dl_hip_group_init_drawn with six non-zero sigmas: the same launches behind twice as many accepted attempts.
The three calls alternate round by round in one process: 3 warm-up rounds, then 21 timed ones; every call is synchronous. Prints
min / quartiles / max per call; --out PATH also writes the lines there."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 3, 21
SIGMA6 = np.array([0.5, 0.5, 0.05, 0.01, 0.01, 0.2618], np.float32)
MEAN7 = np.array([1.0, -2.0, 0.3, 0, 0, 0.0499792, 0.9987503], np.float32)
SEED = 12345


def main():
    from mcl_3dl_amd import capi
    cov = np.diag(SIGMA6.astype(np.float64) ** 2)
    cov[0, 1] = cov[1, 0] = 0.1   # a full block: every product of the kernel is the same work whatever the matrix holds
    T, _ = capi.noise_transform6(cov)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = capi.Group([0])
    for n in (4096, 65536, 450408):
        g.init_drawn_multivariate(MEAN7, T, n, SEED)
        rows, weights = g.download_state()
        calls = [
            ("init_drawn_multivariate", lambda: g.init_drawn_multivariate(MEAN7, T, n, SEED, reset_odom_integ=True)),
            ("upload_state of host rows", lambda: g.upload_state(rows, weights)),
            ("init_drawn, six sigmas", lambda: g.init_drawn(MEAN7, SIGMA6, n, SEED)),
        ]
        ts = {name: [] for name, _ in calls}
        for r in range(WARM + REPS):
            for name, f in calls:
                t = time.perf_counter()
                f()
                dt = (time.perf_counter() - t) * 1e3
                if r >= WARM:
                    ts[name].append(dt)
        say("%d particles" % n)
        for name, _ in calls:
            q = np.percentile(ts[name], [0, 25, 50, 75, 100])
            say("  %-26s: min %.4f q1 %.4f median %.4f q3 %.4f max %.4f ms" % ((name,) + tuple(q)))
        med = {name: float(np.median(v)) for name, v in ts.items()}
        say("  multivariate / init_drawn = %.3f, multivariate / upload_state = %.3f"
            % (med["init_drawn_multivariate"] / med["init_drawn, six sigmas"],
               med["init_drawn_multivariate"] / med["upload_state of host rows"]))
    g.close()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
