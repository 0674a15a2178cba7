"""mcl3dl_hip_scan_finish_drawn_normal against the long way round on a clipped cloud of about 65 000 points, at
96 + 3 and at 16 384 + 512 sampled points: host wall time per call over ten calls after a warm-up.

  drawn      scan_finish_drawn_normal: normals -> weights -> cumulative weights -> draws -> order -> gather -> scan order, one call
  long way   scan_normal_weights for both models (weights come home, the host runs the recurrence) + scan_finish with the ids;
             the host's own draw (std::unordered_set loop) is NOT in the figure: it is made once, by tests/cpp/rng_weighted_emul.cpp,
             and its time as a child process is printed on a line of its own
Run it under rocprofv3 --kernel-trace --stats for the kernel times (weighted_cumulative_kernel, weighted_single_kernel,
weighted_draw / flag / emit / phase kernels)."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import rng_weighted_ref as rwr  # noqa: E402
from mcl_3dl_amd import capi  # noqa: E402
from mcl_3dl_amd.synthetic import make_config  # noqa: E402

R, FPC, MAX_WEIGHT = 0.4, np.array([0.8, 0.6, 0.0], np.float32), 5.0
sc = make_config("C3", seed=12345)
rng = np.random.default_rng(4)
raw = np.concatenate([sc.scan_lik + rng.normal(0, 0.02, sc.scan_lik.shape).astype(np.float32) for _ in range(4)], 0)[:65536]
raw = np.ascontiguousarray(raw, np.float32)
origins = np.zeros((1, 3), np.float32)
eng = capi.Engine(0)
cl, cb = (0.5, 10.0, -2.0, 2.0), (0.5, 4.0, -2.0, 2.0)
N, WARM, STATE = 10, 3, 12345
rwr.emul_exe()  # compiled before anything is timed


def timed(f):
    t = []
    for _ in range(N + WARM):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return np.array(t[WARM:]) * 1e3


n_full, n_lik, n_beam = eng.scan_begin(raw, None, leaf=None, clip_lik=cl, clip_beam=cb)
print("%d points in, %d / %d in the clipped likelihood / beam cloud" % (len(raw), n_lik, n_beam))
for n_s, n_b in ((96, 3), (16384, 512)):
    cum_b = eng.scan_normal_weights(2, R, FPC, MAX_WEIGHT)[0]
    cum_l = eng.scan_normal_weights(1, R, FPC, MAX_WEIGHT)[0]
    t0 = time.perf_counter()
    ids_b, st, draws_b, _ = rwr.draw("std", STATE, cum_b, n_b)
    ids_l, st, draws_l, _ = rwr.draw("std", st, cum_l, n_s)
    t_host = (time.perf_counter() - t0) * 1e3
    got = eng.scan_finish_drawn_normal(n_s, n_b, origins, R, FPC, MAX_WEIGHT, STATE)
    assert got == (n_s, n_b, st), (got, st)
    drawn = [eng.scan_download(k)[0] for k in (5, 6)]

    def long_way():
        eng.scan_normal_weights(2, R, FPC, MAX_WEIGHT)
        eng.scan_normal_weights(1, R, FPC, MAX_WEIGHT)
        eng.scan_finish(ids_l, ids_b, origins=origins)

    long_way()
    for a, b in zip(drawn, [eng.scan_download(k)[0] for k in (5, 6)]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    t_new = timed(lambda: eng.scan_finish_drawn_normal(n_s, n_b, origins, R, FPC, MAX_WEIGHT, STATE))
    t_old = timed(long_way)
    print("%d + %d points (%d + %d attempts): drawn %.3f ms per call (min %.3f, max %.3f); long way round without the host's draw "
          "%.3f ms (min %.3f, max %.3f); the host's draw as two child processes %.1f ms; scans equal"
          % (n_s, n_b, draws_l, draws_b, t_new.mean(), t_new.min(), t_new.max(), t_old.mean(), t_old.min(), t_old.max(), t_host))
# the chain alone, through the stand-alone call (upload of the weights and download of the cumulative array included)
w = np.diff(cum_l, prepend=0.0)
t = timed(lambda: eng.rng_draw_weighted(w, 0))
print("cumulative weights of %d points through rng_draw_weighted(num = 0), copies included: %.3f ms per call (min %.3f)"
      % (len(w), t.mean(), t.min()))
for num in (96, 1109, 1110, 16384):
    t = timed(lambda: eng.rng_draw_weighted(w, num, STATE))
    print("rng_draw_weighted num = %d of %d, copies included: %.3f ms per call (min %.3f)" % (num, len(w), t.mean(), t.min()))
