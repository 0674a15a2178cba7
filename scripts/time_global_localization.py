"""Global localisation on bench config C2's map (hollow cube n = 408: 998 784 points), grid 0.3, div_yaw 12, dist_weight (1, 1, 5):
the engine path, the oracle composition on the CPU, and the long way round through the ABI as it was before this entry point."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch  # noqa: F401
from mcl_3dl_amd import capi
from mcl_3dl_amd.synthetic import cube_map
F = np.float32
GRID, DIV, DW = 0.3, 12, (1.0, 1.0, 5.0)
profile_only = "--profile" in sys.argv
m = cube_map(408, 0.1)
g = capi.Group([0])
g.set_map(m, None, stamp=1, dist_weight=DW); g.set_likelihood_params(); g.set_beam_params()
t = time.perf_counter(); n_pts, n_p = g.global_localization(GRID, DIV); first = time.perf_counter() - t
print("map %d points -> %d standable points x %d = %d particles; first call %.2f ms (uploads the map as a device cloud)" % (len(m), n_pts, DIV, n_p, first * 1e3))
calls = []
for _ in range(3 if profile_only else 10):
    t = time.perf_counter(); g.global_localization(GRID, DIV); calls.append((time.perf_counter() - t) * 1e3)
print("engine: mcl3dl_hip_group_global_localization wall ms per call (ends in a synchronise): min %.3f median %.3f max %.3f" % (min(calls), float(np.median(calls)), max(calls)))
if profile_only:
    sys.exit(0)
got_s, got_w = g.download_state()
import global_loc_ref as glr
# (i) the oracle composition on the CPU
t = time.perf_counter(); pts = glr.standable_points(m, GRID, DW)[0]; st, w = glr.particles(pts, DIV); cpu = time.perf_counter() - t
print("oracle composition on the CPU (VoxelGrid + kd-tree stand-in + search + expansion): %.1f ms" % (cpu * 1e3))
assert np.array_equal(got_s, st) and np.array_equal(got_w, w)
# (ii) the long way round: second context to index the centroids, two downloads, host expansion, state upload
e = capi.Engine(0); e.set_map(m, None, stamp=1, dist_weight=DW)
e2 = capi.Engine(0); g2 = capi.Group([0]); g2.set_map(m, None, stamp=1, dist_weight=DW)
rot = glr.rotations(DIV)
def long_way():
    base, _ = e.map_download()
    e2.set_map_downsampled(base, None, leaf=(GRID, GRID, GRID), stamp=2, dist_weight=DW)
    c, _ = e2.map_download()
    q = c.copy(); q[:, 2] = (q[:, 2].astype(np.float64) + (0.01 + GRID)).astype(F)
    idx, _ = e2.radius_search(q, GRID)
    p = c[idx < 0]
    s = np.zeros((len(p) * DIV, 13), F); s[:, :3] = np.repeat(p, DIV, 0); s[:, 3:7] = np.tile(rot, (len(p), 1))
    ww = np.full(len(s), F(1.0 / F(len(p))), F)
    g2.upload_state(s, ww)
    return s, ww
long_way()
lw = []
for _ in range(5):
    t = time.perf_counter(); s, ww = long_way(); lw.append((time.perf_counter() - t) * 1e3)
assert np.array_equal(s, st) and np.array_equal(ww, w)
print("long way round (map_download + set_map_downsampled on a 2nd context + map_download + radius_search + host expansion + upload_state) wall ms: min %.1f median %.1f max %.1f" % (min(lw), float(np.median(lw)), max(lw)))
