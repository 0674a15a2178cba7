"""Seeded long-map cases for tests/test_gpu_long_map.py (numpy only): maps whose candidate grid has tens of thousands of
voxels along one axis, and the queries at which a voxel index rounded the wrong way changes the answer.

The maps are "stations" along a corridor — clusters of uniformly scattered points in a 3 m x 2 m cross-section, 2 m long, at 0,
1 030, 1 800, 2 060 and 2 200 m — so the sparse index stays small. Behind the last station lies a zone that holds only
constructed TRIPLES (q, p, p'), all in the rescaled (dist_weight) coordinates the index works in:
  q   a float the kernels' float expression floor((q - o) * inv_e) puts in a voxel V although q lies outside V grown by 1e-3 of
      an edge (the slack before it was derived from the voxel count);
  p   the nearest map point of q in fp64, on the far side of q from V;
  p'  on V's side, farther from q than p — by at least 1e-6 relative in d^2 — yet nearer than p by more than 1.5 x the
      compiler's domination margin at every point of that grown box of V.
A compiler that believes q to lie in that box discards p from V's candidates (rule 3 of map_compiler.h) and the kernel answers
|q - p'|. The generator checks every property in fp64 from the float coordinates and asserts that it found at least MIN_TRIPLES.

cand_geometry restates mcl_3dl_amd/csrc/index_geometry.h in numpy float32 / float64; the GPU test compares it with the geometry
the engine reports (Engine.index_geometry) before it relies on either."""
import numpy as np

F = np.float32
MIN_TRIPLES = 64
MAX_TRIPLES = 256
VOXEL_RATIO = 0.5
PHASE = 0.5

VARIANTS = {
    "along_x": dict(axis=0),
    "along_y": dict(axis=1),
    "along_z": dict(axis=2),
    # (far from the coordinate origin q - o is exact and the product alone rounds: the voxel index passes the fixed slack only
    # beyond 32 768 voxels, so this corridor is longer)
    "shifted": dict(axis=0, shift=(1.0e4, -2.0e4, 30.0), stations=(0.0, 1030.0, 1800.0, 2060.0, 2200.0, 3300.0)),
    "dist_weight": dict(axis=0, dist_weight=(2.0, 1.5, 3.0)),
    "r005": dict(axis=0, r=0.05, stations=(0.0, 415.0, 520.0, 830.0), far_from=520.0),
}


def cand_geometry(r, ratio, stretch, phase, mn, mx):
    """index_geometry.h:cand_grid_geometry for bounds mn .. mx (float32, rescaled): origin (float32), edges (fp64 of floats),
    their float32 reciprocals, voxel counts, reach and grow."""
    r = float(F(r))
    e = [F(r * ratio * s) for s in stretch]
    ed = np.array([float(x) for x in e])
    inv = np.array([F(1.0) / x for x in e], F)
    e_min = ed.min()
    r_hi = r * (1.0 + 1e-5)
    mn64, mx64 = np.asarray(mn, np.float64), np.asarray(mx, np.float64)
    reach_hi = np.floor((r_hi + 2.0 * (1.0 / 16.0) * e_min) / ed) + 1.0
    length = ((mx64 - mn64) + (2.0 * reach_hi + 6.0) * ed).max()
    max_abs = max(np.abs(mn64).max(), np.abs(mx64).max())
    derived = 3.25 / 16777216.0 * length + (max_abs + length) / 1125899906842624.0
    assert derived <= e_min / 16.0, "the engine refuses this grid"
    grow = max(1e-3 * e_min, derived)
    reach = (np.floor((r_hi + 2.0 * grow) / ed)).astype(np.int64) + 1
    o = np.array([F(mn[a]) - F((reach[a] + 1 + phase) * ed[a]) for a in range(3)], F)
    nv = (np.floor((mx64 - o.astype(np.float64)) / ed)).astype(np.int64) + reach + 2
    return dict(origin=o, edge=ed, inv=inv, voxels=nv, reach=reach, grow=grow, grow_fixed=1e-3 * e_min, r=r)


def voxel_of(geom, q, axis):
    """The kernels' float expression along one axis, in float32."""
    q = np.asarray(q, F)
    return np.floor((q - geom["origin"][axis]) * geom["inv"][axis]).astype(np.int64)


def rescale(xyz, w):
    """PointRepresentation::vectorize: one float product per coordinate."""
    xyz = np.asarray(xyz, F)
    return xyz if w is None else (xyz * np.asarray(w, F)[None, :]).astype(F)


def step(q, k):
    """q moved by k floats (k may be negative)."""
    q = np.array(q, F)
    for _ in range(abs(int(k))):
        q = np.nextafter(q, F(np.inf if k > 0 else -np.inf))
    return q


def _misindexed(geom, axis, lo, hi):
    """Per face of `axis` between the rescaled coordinates lo and hi: the float (within 4 floats of the face) that lies farthest
    outside the fixed-slack box of the voxel the float expression gives it. Returns (q, voxel, side, excess): side = +1 when
    the box lies above q, -1 when below; excess = distance from q to the box."""
    o, e, g0 = float(geom["origin"][axis]), geom["edge"][axis], geom["grow_fixed"]
    k = np.arange(int(np.ceil((lo - o) / e)), int(np.floor((hi - o) / e)) + 1)
    base = (o + k * e).astype(F)
    best = None
    for s in range(-4, 5):
        q = step(base, s)
        v = voxel_of(geom, q, axis)
        below = (o + v * e - g0) - q.astype(np.float64)          # > 0: q lies below its voxel's box
        above = q.astype(np.float64) - (o + (v + 1) * e + g0)    # > 0: above
        excess = np.maximum(below, above)
        side = np.where(below > above, 1, -1)
        if best is None:
            best = [q.copy(), v.copy(), side.copy(), excess.copy()]
        else:
            m = excess > best[3]
            for b, x in zip(best, (q, v, side, excess)):
                b[m] = x[m]
    keep = best[3] > 0
    return [b[keep] for b in best]


def _box_min_gap(geom, vox, p, pp):
    """min over the fixed-slack box of voxel `vox` of |x - p|^2 - |x - pp|^2 (fp64; linear in x: attained at a corner)."""
    o, e, g0 = geom["origin"].astype(np.float64), geom["edge"], geom["grow_fixed"]
    ctr = o + (np.asarray(vox, np.float64) + 0.5) * e
    half = 0.5 * e + g0
    a, b = np.asarray(p, np.float64) - ctr, np.asarray(pp, np.float64) - ctr
    return float(a @ a - b @ b - np.sum(half * np.abs(2.0 * (b - a))))


def make_case(name, seed=0):
    """-> dict(map_xyz, dist_weight, r, geom, triples_q, triple_points (indices of p and p' in the map), far (axial ranges of the
    far stations, unscaled), axis, stations, lateral (the cross-section's bounds, unscaled))."""
    spec = VARIANTS[name]
    rng = np.random.default_rng([seed, sorted(VARIANTS).index(name)])
    axis = spec["axis"]
    lat = [a for a in range(3) if a != axis]
    r = spec.get("r", 0.2)
    stations = spec.get("stations", (0.0, 1030.0, 1800.0, 2060.0, 2200.0))
    far_from = spec.get("far_from", 1800.0)
    shift = np.asarray(spec.get("shift", (0.0, 0.0, 0.0)), np.float64)
    w = spec.get("dist_weight")
    w64 = np.ones(3) if w is None else np.asarray(w, np.float64)
    zone_len = 200.0 * r                       # behind the last station: the triples' own zone
    zone_lo = stations[-1] + 2.0 + 4.0 * r
    cross = (3.0, 2.0)

    def place(axial, c0, c1):
        p = np.empty((len(axial), 3))
        p[:, axis], p[:, lat[0]], p[:, lat[1]] = axial, c0, c1
        return (p + shift).astype(F)

    # Two corner points pin the bounds, so that the grid does not depend on what the triples add. Which floats the voxel
    # expression rounds the wrong way depends on the phase of the grid's origin against the float lattice out there: the low
    # corner's corridor coordinate is the one of a few that leaves the most mis-indexed floats in the zone.
    zl, zh = (zone_lo + shift[axis]) * w64[axis], (zone_lo + zone_len + shift[axis]) * w64[axis]
    best = None
    for low in (-0.35, -0.1, -0.3, -0.05, -0.2, -0.02, -0.27, -0.123):
        corners = place(np.array([low, zone_lo + zone_len + 4.0 * r]), np.array([0.0, cross[0]]), np.array([0.0, cross[1]]))
        sc = rescale(corners, w)
        geom = cand_geometry(r, VOXEL_RATIO, (1.0, 1.0, 1.0), PHASE, sc.min(0), sc.max(0))
        found = _misindexed(geom, axis, zl + r, zh - r)
        score = int(np.sum(found[3] > 1e-4 * r))
        if best is None or score > best[0]:
            best = (score, corners, geom, found)
    _, corners, geom, (mq, mv, ms, mx_) = best
    n_st = 1500
    parts = [place(s + rng.uniform(0.0, 2.0, n_st), rng.uniform(0.0, cross[0], n_st), rng.uniform(0.0, cross[1], n_st))
             for s in stations]
    base = np.concatenate([corners] + parts, 0)
    sb = rescale(base, w)
    mn, mx = sb.min(0), sb.max(0)
    assert np.array_equal(mn, rescale(corners, w).min(0)) and np.array_equal(mx, rescale(corners, w).max(0))
    o, e, g0 = geom["origin"].astype(np.float64), geom["edge"], geom["grow_fixed"]
    margin = 1e-5 * geom["r"] ** 2
    # mis-indexed floats along the corridor inside the zone, at least 4 r apart (triples must not see each other)
    order = np.argsort(-mx_)
    layers = []
    for i in order:                            # the farthest outside first
        if all(abs(float(mq[i]) - float(mq[j])) >= 4.0 * r for j in layers):
            layers.append(i)
    # the cross-section's slots, 4 r apart; f = the lateral axis with the finer floats carries the offset c
    f = lat[0] if np.abs(sb[:, lat[0]]).max() <= np.abs(sb[:, lat[1]]).max() else lat[1]
    g = lat[1] if f == lat[0] else lat[0]
    slots = [(jf, jg)
             for jf in range(int(np.ceil((mn[f] + r - o[f]) / e[f])), int((mx[f] - r - o[f]) / e[f]), int(np.ceil(4.0 * r / e[f])))
             for jg in range(int(np.ceil((mn[g] + r - o[g]) / e[g])), int((mx[g] - r - o[g]) / e[g]), int(np.ceil(4.0 * r / e[g])))]
    tq, tp, tpp, rel = [], [], [], []
    for i in layers:
        for jf, jg in slots:
            if len(tq) >= MAX_TRIPLES:
                break
            q = np.empty(3, F)
            q[axis] = mq[i]
            q[f] = F(o[f] + (jf + 0.01) * e[f])
            q[g] = F(o[g] + (jg + 0.5) * e[g])
            vox = np.empty(3, np.int64)
            vox[axis], vox[f], vox[g] = mv[i], jf, jg
            a_t = rng.uniform(0.15, 0.6) * r
            p, found = q.copy(), False
            p[axis] = F(float(q[axis]) - ms[i] * a_t)
            a = abs(float(q[axis]) - float(p[axis]))
            for c in r * np.geomspace(0.08, 2e-4, 24):          # the largest lateral offset of p' that passes
                pp = q.copy()
                pp[axis] = F(float(q[axis]) + ms[i] * a)
                pp[f] = F(float(q[f]) + c)
                # back to map coordinates and forth again: the floats the engine will see
                q_u, p_u, pp_u = [(x.astype(np.float64) / w64).astype(F) for x in (q, p, pp)]
                q_s, p_s, pp_s = [rescale(x[None], w)[0] for x in (q_u, p_u, pp_u)]
                if not all(voxel_of(geom, q_s[a_], a_) == vox[a_] for a_ in range(3)):
                    continue
                lo_box = o[axis] + vox[axis] * e[axis] - g0
                hi_box = o[axis] + (vox[axis] + 1) * e[axis] + g0
                if lo_box <= float(q_s[axis]) <= hi_box:
                    continue
                d_p = np.sum((q_s.astype(np.float64) - p_s) ** 2)
                d_pp = np.sum((q_s.astype(np.float64) - pp_s) ** 2)
                if not (d_p < geom["r"] ** 2 * 0.9 and d_pp - d_p >= 1e-6 * d_p):
                    continue
                if not _box_min_gap(geom, vox, p_s, pp_s) > 1.5 * margin:
                    continue
                found = True
                break
            if found:
                tq.append(q_u)
                tp.append(p_u)
                tpp.append(pp_u)
                rel.append((d_pp - d_p) / d_p)
    assert len(tq) >= MIN_TRIPLES, "%s: only %d triples from %d mis-indexed floats in %d layers" % (name, len(tq), len(mq), len(layers))
    tq, tp, tpp = (np.array(x, F) for x in (tq, tp, tpp))
    pairs = np.empty((2 * len(tp), 3), F)
    pairs[0::2], pairs[1::2] = tp, tpp
    map_xyz = np.concatenate([base, pairs], 0)
    assert len(map_xyz) <= 12000
    sm = rescale(map_xyz, w)
    assert np.array_equal(sm.min(0), mn) and np.array_equal(sm.max(0), mx)
    # p is the nearest map point of q, and by a clear distance to everything but p'
    sq = rescale(tq, w).astype(np.float64)
    for k in range(len(tq)):
        d2 = np.sum((sm.astype(np.float64) - sq[k]) ** 2, 1)
        i_p = len(base) + 2 * k
        assert np.argmin(d2) == i_p
        d2[[i_p, i_p + 1]] = np.inf
        assert d2.min() > (2.0 * geom["r"]) ** 2
    far = [(s, s + 2.0) for s in stations if s >= far_from]
    return dict(name=name, map_xyz=map_xyz, n_base=len(base), dist_weight=w, r=r, geom=geom, axis=axis, lateral=(lat, cross),
                shift=shift, triples_q=tq, triples_rel=np.array(rel), far=far, stations=stations, seed=seed,
                n_misindexed=len(mq))


def face_queries(case, geom, n=2000):
    """(a) n floats on and within +-3 floats of voxel faces at the far stations, from the geometry the ENGINE reports (origin,
    edge): the corridor coordinate on a face, a quarter of them with a lateral coordinate on a face too."""
    rng = np.random.default_rng([case["seed"], 1])
    axis, (lat, cross), shift = case["axis"], case["lateral"], case["shift"]
    w64 = np.ones(3) if case["dist_weight"] is None else np.asarray(case["dist_weight"], np.float64)
    o, e = np.asarray(geom["origin"], np.float64), np.asarray(geom["edge"], np.float64)
    st = np.array(case["far"])[rng.integers(0, len(case["far"]), n)]
    q = np.empty((n, 3))
    q[:, axis] = rng.uniform(st[:, 0], st[:, 1])
    q[:, lat[0]] = rng.uniform(0.0, cross[0], n)
    q[:, lat[1]] = rng.uniform(0.0, cross[1], n)
    q = (q + shift) * w64                                   # rescaled
    on_face = np.zeros((n, 3), bool)
    on_face[:, axis] = True
    side = rng.integers(0, 2, n)
    quarter = rng.random(n) < 0.25
    on_face[quarter, np.where(side[quarter] == 0, lat[0], lat[1])] = True
    snapped = o + np.round((q - o) / e) * e
    q = np.where(on_face, snapped, q)
    out = (q / w64).astype(F)
    k = rng.integers(-3, 4, (n, 3))
    for s in range(-3, 4):
        m = on_face & (k == s)
        out[m] = step(out[m], s)
    return out


def near_queries(case, n=2000):
    """(c) n points near random map points."""
    rng = np.random.default_rng([case["seed"], 2])
    pts = case["map_xyz"][rng.integers(0, len(case["map_xyz"]), n)].astype(np.float64)
    w64 = np.ones(3) if case["dist_weight"] is None else np.asarray(case["dist_weight"], np.float64)
    return (pts + rng.normal(0.0, 0.35 * case["r"], (n, 3)) / w64).astype(F)


def posed(queries, centre, n_p=8, seed=0):
    """n_p poses near `centre` with random rotations, and the scan that particle 0 sees `queries` as (float32; the transform
    back lands within a few floats of the queries, which is all the faces ask for)."""
    rng = np.random.default_rng([seed, 3])
    quat = rng.normal(size=(n_p, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    pos = np.asarray(centre, np.float64) + rng.normal(0.0, 0.05, (n_p, 3))
    x, y, z, w_ = quat[0]
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w_), 2 * (x * z + y * w_)],
                    [2 * (x * y + z * w_), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w_)],
                    [2 * (x * z - y * w_), 2 * (y * z + x * w_), 1 - 2 * (x * x + y * y)]])
    scan = ((np.asarray(queries, np.float64) - pos[0]) @ rot).astype(F)   # R^T (q - t)
    poses = np.concatenate([pos, quat], 1).astype(F)
    return poses, scan
