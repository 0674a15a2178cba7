"""Plain numpy restatements of the cloud path's steps, written from their documented definitions and independent of both the
engine and oracle/: pcl::VoxelGrid as the node configures it (the algorithm in the header comment of
oracle/shims/pcl/filters/voxel_grid.h), the clip predicate of both models' filter(), the Morton ordering of the likelihood scan
(mcl_3dl_amd/csrc/cloud_keys.h, api_core.inl:order_scan) and the range ordering of the beam scan.

All arithmetic is float32 with one rounding per operation (numpy never fuses a multiply with an add). test_cloud_ref_cpu.py
pins these functions against the compiled oracle and the host ordering; test_gpu_cloud_edges.py compares the kernels with them."""
import numpy as np

F = np.float32
INT32_MAX = 2**31 - 1
MORTON_BITS = 16      # MCL3DL_MORTON_BITS


def _f32(a, cols=3):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)


def _labels(label, n):
    return np.zeros(n, np.uint32) if label is None else np.ascontiguousarray(label, dtype=np.uint32).reshape(-1)


def finite_rows(xyz):
    return np.isfinite(xyz).all(1)


def voxel_layout(xyz, leaf):
    """Steps 1-3 of the filter: None when no point is finite, otherwise a dict with the finite mask, inv_leaf, the int64
    extents d (+ whether their product overflows int32: pass-through), min_b, div_b, mul and cells = div_b product."""
    xyz = _f32(xyz)
    fin = finite_rows(xyz)
    if not fin.any():
        return None
    inv = F(1.0) / np.asarray(leaf, np.float32)                       # Eigen::Array4f::Ones() / leaf_size
    mn, mx = xyz[fin].min(0), xyz[fin].max(0)
    d = [int(np.trunc(np.float64(e))) + 1 for e in (mx - mn) * inv]   # int64((max - min) * inv_leaf) + 1
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    div_b = max_b - min_b + 1
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], np.int64)
    return dict(finite=fin, inv=inv, d=d, passthrough=d[0] * d[1] * d[2] > INT32_MAX, min_b=min_b, div_b=div_b, mul=mul,
                cells=int(div_b[0]) * int(div_b[1]) * int(div_b[2]))


def voxel_keys(xyz, lay):
    """Leaf index of every finite point, in input order: int(floor(p * inv) - float(min_b)) . mul, as 32-bit unsigned."""
    p = _f32(xyz)[lay["finite"]]
    ijk = (np.floor(p * lay["inv"]) - lay["min_b"].astype(np.float32)).astype(np.int64)   # integer-valued floats: exact cast
    return ((ijk * lay["mul"]).sum(1) & 0xFFFFFFFF).astype(np.uint32)


def voxel_sorted_keys(xyz, leaf):
    """The sorted leaf indices of the finite points (what the centroid kernel walks); None for pass-through / no finite point."""
    lay = voxel_layout(xyz, leaf)
    if lay is None or lay["passthrough"]:
        return None
    return np.sort(voxel_keys(xyz, lay), kind="stable")


def voxel_grid(xyz, label, leaf):
    """(centroids float32 (m, 3), labels uint32 (m,)): one point per occupied leaf in ascending leaf order; xyz = float32 sum
    in input order / float(count); label = the most frequent one, the smallest on a tie. The input itself when the extents'
    product overflows int32; nothing when no point is finite."""
    xyz = _f32(xyz)
    label = _labels(label, len(xyz))
    lay = voxel_layout(xyz, leaf)
    if lay is None:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
    if lay["passthrough"]:
        return xyz.copy(), label.copy()
    key = voxel_keys(xyz, lay)
    order = np.argsort(key, kind="stable")
    key, p, lab = key[order], xyz[lay["finite"]][order], label[lay["finite"]][order]
    head = np.nonzero(np.r_[True, key[1:] != key[:-1]])[0]
    count = np.diff(np.r_[head, len(key)])
    # sequential float32 sums: step j adds the j-th point of every leaf that has one (np.add.reduceat sums pairwise)
    acc = np.zeros((len(head), 3), np.float32)
    longest_first = np.argsort(-count, kind="stable")
    n_with = len(head)
    for j in range(int(count.max())):
        while count[longest_first[n_with - 1]] <= j:
            n_with -= 1
        rows = longest_first[:n_with]
        acc[rows] = acc[rows] + p[head[rows] + j]
    cent = acc / count.astype(np.float32)[:, None]
    # label vote: (leaf, label) pairs counted, then per leaf the highest count, the smallest label among equals
    leaf_id = np.repeat(np.arange(len(head)), count)
    pair = leaf_id.astype(np.uint64) << np.uint64(32) | lab.astype(np.uint64)
    upair, ucount = np.unique(pair, return_counts=True)
    uleaf, ulab = (upair >> np.uint64(32)).astype(np.int64), (upair & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    pick = np.lexsort((ulab, -ucount, uleaf))
    first = np.nonzero(np.r_[True, uleaf[pick][1:] != uleaf[pick][:-1]])[0]
    return cent, ulab[pick][first]


def clip(xyz, near, far, z_min, z_max, label=None):
    """The clip step of both models' filter(): a point is erased when x x + y y > far far, < near near, z < z_min or z_max < z
    (a NaN fails every comparison and is kept); the order is kept. Returns (xyz, label)."""
    xyz = _f32(xyz)
    label = _labels(label, len(xyz))
    near_sq, far_sq = F(near) * F(near), F(far) * F(far)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]
        erase = (r2 > far_sq) | (r2 < near_sq) | (xyz[:, 2] < F(z_min)) | (F(z_max) < xyz[:, 2])
    return xyz[~erase], label[~erase]


def _cell(f):
    """clamp(trunc(f), 0, 1023) of float32 values: negative or NaN -> 0, anything >= 1023 (+inf too) -> 1023."""
    with np.errstate(invalid="ignore"):
        inside = (f >= F(0)) & (f < F(1023))
        top = f >= F(1023)
    return np.where(inside, np.where(inside, f, F(0)).astype(np.uint32), np.where(top, np.uint32(1023), np.uint32(0)))


def _spread10(v):
    out = np.zeros_like(v, dtype=np.uint32)
    for b in range(10):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def morton_keys(xyz):
    xyz = _f32(xyz)
    fin = finite_rows(xyz)
    big = np.finfo(np.float32).max
    mn = xyz[fin].min(0) if fin.any() else np.full(3, big, np.float32)
    mx = xyz[fin].max(0) if fin.any() else np.full(3, -big, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = int(_cell((mx - mn) * F(4)).max())
        drop = max(0, 3 * c.bit_length() - MORTON_BITS)
        q = _cell((xyz - mn) * F(4))
    return (_spread10(q[:, 0]) | (_spread10(q[:, 1]) << np.uint32(1)) | (_spread10(q[:, 2]) << np.uint32(2))) >> np.uint32(drop)


def morton_order(xyz):
    """order[k] = index of the point the engine holds at position k of the likelihood scan."""
    return np.argsort(morton_keys(xyz), kind="stable").astype(np.uint32)


def range_order(xyz, origin_id, origins):
    """Beam scan order: ascending (dx dx + dy dy) + dz dz from the point's own origin, ties by index."""
    xyz, origins = _f32(xyz), _f32(origins)
    d = xyz - origins[np.asarray(origin_id, np.int64)]
    key = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.argsort(key, kind="stable").astype(np.uint32)
