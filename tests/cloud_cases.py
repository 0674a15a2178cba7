"""The inputs of test_gpu_cloud_edges.py, shared with test_cloud_ref_cpu.py (which runs the numpy restatements of
cloud_ref.py over the very same clouds against the compiled oracle and the host ordering). Every builder is seeded and cached;
callers must not write into what they get."""
import functools

import numpy as np

F = np.float32
BOX = np.array([12.0, 9.0, 2.8])
LEAF_BOX = (0.5, 0.5, 0.5)

VG_SIZES = [2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537, 524288, 524289]
VG_KEY_WIDTHS = {            # occupied extent in cells -> its three factors (x, y, z): 1, 2, 3 and 4 radix passes
    255: (255, 1, 1), 256: (16, 16, 1), 257: (257, 1, 1), 65535: (255, 257, 1), 65536: (256, 256, 1), 65537: (65537, 1, 1),
    2**24 - 1: (255, 273, 241), 2**24: (256, 256, 256), 257 * 256 * 256: (257, 256, 256)}
LIK_SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 65535, 65536, 65537, 524288, 524289]
LIK_NONFINITE = (65, 2049, 65537)     # these scans carry NaN / +-inf points
LIK_WIDE = 4096                       # this one is wider than 256 m: cells clamp at 1023
LIK_HOST_MAX = 65537
BEAM_SIZES = [2047, 2048, 2049, 4097, 65537]
BEAM_ORIGINS = np.array([[0.0, 0.0, 0.5], [0.125, -0.25, 0.5], [-0.5, 0.375, 0.625]], np.float32)
CLIP_SIZES = [1023, 1024, 1025, 4096, 4097]


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- VoxelGrid ----------------------------------------------------------------------------------------------------------
def box_points(rng, n):
    return ((rng.random((n, 3)) - 0.5) * BOX).astype(np.float32)


@functools.lru_cache(maxsize=None)
def vg_size(n):
    """n points in a 12 x 9 x 2.8 m box (leaf 0.5: 2592 leaves, runs that cross block edges), an eighth of them exact
    duplicates, labels from 4 values, one NaN and one inf coordinate (n_finite = n - 2: the centroid kernel's block edges are
    not the sort's)."""
    rng = np.random.default_rng(1000 + n)
    xyz = box_points(rng, n)
    xyz[n // 2:n // 2 + n // 8] = xyz[:n // 8]
    label = rng.integers(0, 4, n).astype(np.uint32)
    if n >= 63:
        xyz[n // 3, 1] = np.nan
        xyz[2 * n // 3, 0] = np.inf
    return _ro(xyz, label) + (LEAF_BOX,)


def _layers(rng, below, one_leaf, above):
    """`below` points under z = 0, `one_leaf` points in the leaf [0, 0.5)^3, `above` points over z = 0.5, shuffled: z carries the
    largest multiplier of the leaf index, so the sorted order is below | the one leaf | above."""
    a = box_points(rng, below)
    a[:, 2] = -0.01 - np.abs(a[:, 2])
    b = (rng.random((one_leaf, 3)) * 0.49 + 0.005).astype(np.float32)
    c = box_points(rng, above)
    c[:, 2] = 0.51 + np.abs(c[:, 2])
    xyz = np.concatenate([a, b, c])
    kind = np.r_[np.zeros(below, int), np.ones(one_leaf, int), np.full(above, 2)]
    perm = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[perm]), kind[perm]


@functools.lru_cache(maxsize=None)
def vg_run(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "leaf_5000_in_9000":        # sorted entries 2000 .. 6999 are one leaf: four work-groups without any head
        xyz, kind = _layers(rng, 2000, 5000, 2000)
        label = np.where(kind == 1, 2, rng.integers(0, 4, len(xyz))).astype(np.uint32)
    elif name == "leaf_3000":              # one leaf only: work-groups 1 and 2 hold no head
        xyz, kind = _layers(rng, 0, 3000, 0)
        label = np.full(3000, 3, np.uint32)
    elif name == "leaf_600_voted":         # a 600-point leaf across the first block edge (entries 800 .. 1399), label vote
        xyz, kind = _layers(rng, 800, 600, 700)          # with an exact tie between labels 1 and 2 (250 each) over label 3
        label = rng.integers(0, 4, len(xyz)).astype(np.uint32)
        label[kind == 1] = rng.permutation(np.r_[np.full(250, 2), np.full(250, 1), np.full(100, 3)]).astype(np.uint32)
    elif name == "own_leaf_4000":          # 4000 leaves of one point
        g = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
        xyz = ((g - np.array([10, 10, 5]) + rng.uniform(0.1, 0.9, g.shape)) * 0.5).astype(np.float32)
        xyz = np.ascontiguousarray(xyz[rng.permutation(len(xyz))])
        label = rng.integers(0, 4, len(xyz)).astype(np.uint32)
    elif name == "heads_on_1023_and_1024":  # a one-point leaf on sorted entry 1023 (a block's last), the next head on 1024
        xyz, kind = _layers(rng, 1023, 1, 1500)
        label = rng.integers(0, 4, len(xyz)).astype(np.uint32)
    else:
        raise KeyError(name)
    return _ro(xyz, label) + (LEAF_BOX,)


VG_RUNS = ["leaf_5000_in_9000", "leaf_3000", "leaf_600_voted", "own_leaf_4000", "heads_on_1023_and_1024"]


@functools.lru_cache(maxsize=None)
def vg_key_width(cells):
    """6000 points in 0.5 m leaves whose occupied extent is exactly `cells` leaves (two pinned corners), a quarter of them
    crowded into ten leaves, one NaN and one inf (their key is `cells` itself: one more bit when that is a power of two)."""
    dims = np.array(VG_KEY_WIDTHS[cells])
    rng = np.random.default_rng(cells % 100003)
    first = np.array([-7, -3, -2])
    cell = rng.integers(0, dims, (6000, 3))
    cell[:1500] = cell[rng.integers(0, 10, 1500)]
    frac = rng.uniform(0.1, 0.9, (6000, 3))
    cell[0], frac[0] = 0, 0.05
    cell[1], frac[1] = dims - 1, 0.95
    xyz = ((cell + first + frac) * 0.5).astype(np.float32)
    xyz[100, 2] = np.nan
    xyz[200, 1] = -np.inf
    label = rng.integers(0, 4, 6000).astype(np.uint32)
    return _ro(xyz, label) + (LEAF_BOX,)


@functools.lru_cache(maxsize=None)
def vg_arith(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("on_boundaries_0.25", "on_boundaries_0.1"):     # k * step, both sides of zero, leaf = step
        step = F(0.25) if name.endswith("0.25") else F(0.1)
        k = rng.integers(-20, 21, (3000, 3))
        k[:, 2] = rng.integers(-5, 6, 3000)
        xyz = k.astype(np.float32) * step
        leaf = (float(step),) * 3
    elif name == "far_from_origin":                              # the box moved to (1e4, -2e4, 50), leaf 0.1
        xyz = box_points(rng, 5000) + np.array([1e4, -2e4, 50.0], np.float32)
        leaf = (0.1, 0.1, 0.1)
    elif name in ("extent_filtered_0.147", "extent_passthrough_0.14"):
        # the same 400 x 400 x 40 m cloud: extents' product 2 022 734 532 (filtered) resp. 2 336 094 904 (> INT32_MAX: handed back)
        xyz = ((np.random.default_rng(77).random((6000, 3)) - 0.5) * np.array([400.0, 400.0, 40.0])).astype(np.float32)
        xyz[0], xyz[1] = (-200.0, -200.0, -20.0), (200.0, 200.0, 20.0)
        xyz[3000:3400] = xyz[10:410]
        xyz[500, 0] = np.nan
        leaf = (0.147,) * 3 if name.endswith("0.147") else (0.14,) * 3
    else:
        raise KeyError(name)
    label = rng.integers(0, 4, len(xyz)).astype(np.uint32)
    return _ro(np.ascontiguousarray(xyz, dtype=np.float32), label) + (leaf,)


VG_ARITH = ["on_boundaries_0.25", "on_boundaries_0.1", "far_from_origin", "extent_filtered_0.147", "extent_passthrough_0.14"]


@functools.lru_cache(maxsize=None)
def vg_degenerate(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    xyz = box_points(rng, 3000)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    keep = (700, 2100) if name == "two_finite" else ()
    for i in range(3000):
        if i not in keep:
            xyz[i, rng.integers(0, 3)] = bad[rng.integers(0, 3)]
    label = rng.integers(0, 4, 3000).astype(np.uint32)
    return _ro(xyz, label) + (LEAF_BOX,)


VG_DEGENERATE = ["all_non_finite", "two_finite"]


def vg_all_cases():
    """(id, builder) of every VoxelGrid input"""
    out = [("size_%d" % n, functools.partial(vg_size, n)) for n in VG_SIZES]
    out += [("run_" + k, functools.partial(vg_run, k)) for k in VG_RUNS]
    out += [("cells_%d" % c, functools.partial(vg_key_width, c)) for c in VG_KEY_WIDTHS]
    out += [("arith_" + k, functools.partial(vg_arith, k)) for k in VG_ARITH]
    out += [("degenerate_" + k, functools.partial(vg_degenerate, k)) for k in VG_DEGENERATE]
    return out


def pointcloud2_bytes(xyz, label, step=32, off=(4, 8, 12), off_label=24):
    """little-endian PointCloud2 rows: x, y, z FLOAT32 at `off`, label UINT32 at off_label, the rest of a row filled with 0xA5"""
    buf = np.full((len(xyz), step), 0xA5, np.uint8)
    for a in range(3):
        buf[:, off[a]:off[a] + 4] = np.ascontiguousarray(xyz[:, a], dtype="<f4").view(np.uint8).reshape(-1, 4)
    buf[:, off_label:off_label + 4] = np.ascontiguousarray(label, dtype="<u4").view(np.uint8).reshape(-1, 4)
    return buf.tobytes()


# ---- clips --------------------------------------------------------------------------------------------------------------
# A lattice the VoxelGrid hands back point for point and in input order: two columns (x = 0.05 / 50.05) of rows 0.01 m apart in y,
# one leaf of (0.004, 0.004, 10) each, generated in ascending leaf order; z is free inside [0, 10). What a clip keeps is then
# the same set of INDICES with the filter in front (count on the device) and without it (count from the host).
CLIP_LEAF = (0.004, 0.004, 10.0)
CLIP_PATTERNS = {
    # name: ((near, far, z_min, z_max) likelihood, beam), what the likelihood / beam model keeps
    "keep_all": ((0.0, 100.0, 0.0, 9.5), (0.01, 90.0, -1.0, 9.0), "all", "all"),
    "none_and_every_other": ((200.0, 300.0, 0.0, 9.5), (0.0, 45.0, 0.0, 9.5), "none", "even"),
    "every_other_and_none": ((0.0, 45.0, 0.0, 9.5), (0.0, 100.0, 9.6, 9.9), "even", "none"),
    "only_the_last": ((0.0, 100.0, 3.0, 9.5), (0.0, 100.0, 0.0, 2.0), "last", "all_but_last"),
}


@functools.lru_cache(maxsize=None)
def clip_lattice(n, last_z=5.0):
    i = np.arange(n)
    xyz = np.stack([np.where(i % 2 == 0, 0.05, 50.05), 0.001 + 0.01 * (i // 2), 0.5 + 0.001 * (i % 1000)], 1).astype(np.float32)
    xyz[-1, 2] = last_z
    label = (i % 3).astype(np.uint32)
    return _ro(xyz, label)


def clip_pattern_mask(kind, n):
    i = np.arange(n)
    return {"all": i >= 0, "none": i < 0, "even": i % 2 == 0, "last": i == n - 1, "all_but_last": i < n - 1}[kind]


CLIP_EDGE_LIK = (1.25, 5.0, -1.5, 2.25)      # near, far, z_min, z_max: squares and sums below are exact in float32
CLIP_EDGE_BEAM = (2.5, 6.5, 0.25, 1.75)


@functools.lru_cache(maxsize=None)
def clip_threshold_cloud(with_nan):
    """2000 box points + points exactly ON every threshold of both models (all kept: the comparisons are strict) and their
    float32 neighbours on either side."""
    rng = np.random.default_rng(91)
    xyz = box_points(rng, 2000)
    on = []
    for near, far, z_min, z_max in (CLIP_EDGE_LIK, CLIP_EDGE_BEAM):
        s = far / 5.0
        on += [(3 * s, 4 * s, 1.0), (-4 * s, 3 * s, 1.0), (far, 0.0, 1.0)]            # r^2 == far^2
        s = near / 1.25
        on += [(0.75 * s, 1.0 * s, 1.0), (0.0, -near, 1.0)]                          # r^2 == near^2
        on += [(2.6, 0.5, z_min), (2.6, -0.5, z_max)]
    on = np.array(on, np.float32)
    out = on.copy()
    grow = np.abs(on) > 0
    out[:, :2] = np.where(grow[:, :2], np.nextafter(on[:, :2], np.where(on[:, :2] > 0, np.float32(np.inf), np.float32(-np.inf))), on[:, :2])
    special = np.concatenate([on, out, np.nextafter(on, np.float32(0))])
    xyz = np.concatenate([xyz[:1000], special, xyz[1000:]])
    if with_nan:
        xyz[5] = (np.nan, 1.0, 1.0)
        xyz[6] = (3.0, 0.5, np.nan)       # inside both models' rings: the NaN z passes both z tests
        xyz[7] = (np.nan, np.nan, np.nan)
        xyz[8] = (100.0, np.nan, 1.0)
    label = rng.integers(0, 4, len(xyz)).astype(np.uint32)
    return _ro(np.ascontiguousarray(xyz), label) + (on,)


# ---- scan ordering ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lik_scan(n):
    """A likelihood scan of n points: 20 x 15 x 3 m (1.25 m Morton cells once the key is cut to 16 bits), half of them crowded
    into a handful of cells, an eighth exact duplicates; NaN / +-inf points and a > 256 m wide scan at the sizes named above."""
    rng = np.random.default_rng(5000 + n)
    xyz = ((rng.random((n, 3)) - 0.5) * np.array([20.0, 15.0, 3.0])).astype(np.float32)
    xyz[1::2] *= np.float32(0.1)                   # every other point within 2 x 1.5 x 0.3 m around the middle
    xyz[n // 2:n // 2 + n // 8] = xyz[:n // 8]
    if n == LIK_WIDE:
        xyz[::16] *= np.float32(20.0)            # +-200 m in x: wider than 1023 quarter-metre cells
    if n in LIK_NONFINITE:
        xyz[3, 0] = np.nan
        xyz[n // 2, 2] = np.inf
        xyz[n // 2 + 1, 1] = -np.inf
        xyz[n - 2] = (np.nan, np.inf, -np.inf)
    return _ro(np.ascontiguousarray(xyz))[0]


@functools.lru_cache(maxsize=None)
def beam_scan(n):
    """A finite beam scan of n points on a 1/64 m lattice (origins on a 1/8 m lattice: every range is exact, equal ranges are
    common), with exact duplicates and pairs at equal range from different origins. Returns (xyz, origin id, origins)."""
    rng = np.random.default_rng(7000 + n)
    og = rng.integers(0, 3, n).astype(np.uint32)
    d = np.round((rng.random((n, 3)) - 0.5) * np.array([8.0, 8.0, 2.0]) * 64.0) / 64.0
    m = n // 8
    d[m:2 * m] = d[:m]
    og[m:2 * m] = (og[:m] + 1) % 3               # the same offset from another origin: equal range, different point
    xyz = (d + BEAM_ORIGINS[og]).astype(np.float32)
    xyz[3 * m:4 * m], og[3 * m:4 * m] = xyz[:m], og[:m]   # exact duplicates
    return _ro(np.ascontiguousarray(xyz), og) + (BEAM_ORIGINS,)
