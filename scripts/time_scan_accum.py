"""Wall time of preparing a scan from clouds accumulated on the device — mcl3dl_hip_scan_begin_accumulated on resident pushes
(scan_accum.h, api_cloud.inl) — beside the route that existed before it: mcl3dl_hip_scan_begin on the finished host cloud, its
upload included. The host's two transforms and the concatenation, which the old route also needs, are NOT timed: that favours it.
Sizes a node runs: 2 x 65 536 points (accum_cloud: 2) and 10 x 32 768 (the default total_accum_cloud_max at accum_cloud 1).
One GPU, one process, both routes warmed up and then alternated call by call; each call is synchronous (it returns the three
sizes). Per route: min / quartiles / max over the rounds; the old route's spread is its interquartile range. The time of one push
is reported on its own: until the call returns (the caller's array is free again) and with the stream drained behind it.
  --out PATH : also write the report there (profiles/scan_accum.txt is such a report)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, ROUNDS = 10, 400
LEAF = (0.05, 0.05, 0.05)
CLIP_LIK = (0.5, 10.0, -2.0, 2.0)
CLIP_BEAM = (0.5, 4.0, -2.0, 2.0)
PREP = dict(leaf=LEAF, clip_lik=CLIP_LIK, clip_beam=CLIP_BEAM)


def quartiles(ts):
    q = np.percentile(ts, [0, 25, 50, 75, 100])
    return "min %.4f q1 %.4f median %.4f q3 %.4f max %.4f ms" % tuple(q), float(q[2]), float(q[3] - q[1])


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def main(say):
    import scan_accum_ref as sar
    from mcl_3dl_amd import capi
    from mcl_3dl_amd.synthetic import make_scene
    sc = make_scene(n=91, n_p=64, n_s=20000, n_b=0, seed=43)
    rng = np.random.default_rng(7)
    robot = np.vstack([sar.rigid((0.01, -0.02, 0.8), (250.0, -120.0, 3.0)).astype(np.float64), [0, 0, 0, 1]])
    to_odom, to_base = robot[:3].astype(np.float32), np.linalg.inv(robot)[:3].astype(np.float32)
    eng = capi.Engine(0)
    ok = True
    for n_clouds, n_each in ((2, 65536), (10, 32768)):
        # what the sensor saw: the scene's visible points with range noise, sent back through the robot's pose
        clouds = []
        for _ in range(n_clouds):
            p = sc.scan_lik[rng.integers(0, len(sc.scan_lik), n_each)] + rng.normal(0.0, 0.02, (n_each, 3)).astype(np.float32)
            clouds.append(np.ascontiguousarray(p))
        acc, lab = sar.accumulate(clouds, [to_odom] * n_clouds)
        host_cloud = sar.to_base(acc, to_base)

        def route_a():
            return eng.scan_begin(host_cloud, lab, **PREP)

        def route_b():
            return eng.scan_begin_accumulated(to_base, **PREP)

        eng.scan_accum_clear()
        for c in clouds:
            eng.scan_accum_push(c, to_odom)
        eng.synchronize()
        assert route_a() == route_b()
        for _ in range(WARM):
            route_a()
            route_b()
        ta, tb = [], []
        for _ in range(ROUNDS):
            ta.append(timed(route_a))
            tb.append(timed(route_b))
        text_a, med_a, spread_a = quartiles(ta)
        text_b, med_b, _ = quartiles(tb)
        sizes = route_b()
        say("%d clouds x %d points = %d, prepared %d / %d / %d" % ((n_clouds, n_each, len(host_cloud)) + sizes))
        say("  A  scan_begin on the finished host cloud (upload included) : " + text_a)
        say("  B  scan_begin_accumulated on resident pushes               : " + text_b)
        verdict = med_b <= med_a + spread_a
        ok = ok and verdict
        say("  B median - A median = %+.4f ms; A's interquartile range %.4f ms: %s"
            % (med_b - med_a, spread_a, "B is not above A beyond A's spread" if verdict else "B IS ABOVE A BEYOND A's SPREAD"))
        # one push: a window's worth after a clear, so that the buffer is in place (what a running node sees)
        t_ret, t_sync = [], []
        for _ in range(WARM + 10):
            eng.scan_accum_clear()
            for c in clouds:
                t = time.perf_counter()
                eng.scan_accum_push(c, to_odom)
                t1 = time.perf_counter()
                eng.synchronize()
                t2 = time.perf_counter()
                t_ret.append((t1 - t) * 1e3)
                t_sync.append((t2 - t) * 1e3)
        skip = WARM * n_clouds
        say("  one push of %d points, until the call returns                : %s" % (n_each, quartiles(t_ret[skip:])[0]))
        say("  one push of %d points, with the stream drained behind it     : %s" % (n_each, quartiles(t_sync[skip:])[0]))
    eng.close()
    return ok


if __name__ == "__main__":
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    good = main(say)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if good else 1)
