"""The numpy float32 restatement of the cloud accumulation (mcl_3dl_amd/csrc/scan_accum.h): accumCloud's sensor -> odom transform
with label = cloud index (src/mcl_3dl.cpp:274-302) and measure()'s odom -> base_link transform of the whole accumulation
(:319-336). One expression per output row, every product and sum rounded to float32 on its own:

    out[r] = ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3]

numpy's float32 array arithmetic rounds every operation and never fuses; tests/test_scan_accum_cpu.py holds this file against
mcl_3dl_amd/csrc/scan_accum.h compiled for the host and against float64 within gamma_4."""
import numpy as np

F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32
GAMMA4 = 4 * U / (1 - 4 * U)        # each of the four terms passes through at most four roundings


def affine_apply(m, xyz):
    """m: None (the bits are copied) or the 3x4 [R | t] (any shape holding its twelve floats, row by row); xyz: (n, 3)."""
    p = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    if m is None:
        return p.copy()
    m = np.asarray(m, dtype=F).reshape(-1)[:12].reshape(3, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def accumulate(clouds, affines):
    """pc_local_accum_: (xyz in the odom frame, label = index of the cloud), in push order."""
    xyz = [affine_apply(m, c) for c, m in zip(clouds, affines)]
    lab = [np.full(len(c), k, np.uint32) for k, c in enumerate(xyz)]
    if not xyz:
        return np.zeros((0, 3), F), np.zeros(0, np.uint32)
    return np.concatenate(xyz, 0), np.concatenate(lab, 0)


def to_base(xyz, affine):
    """The accumulation in base_link: the second transform, applied to the stored floats (never composed with the first)."""
    return affine_apply(affine, xyz)


def affine_bound(m, xyz):
    """(real-number result in float64, gamma_4 (|m0 x| + |m1 y| + |m2 z| + |t|)) per coordinate."""
    m = np.asarray(m, dtype=F).reshape(-1)[:12].reshape(3, 4).astype(np.float64)
    p = np.asarray(xyz, dtype=F).astype(np.float64)
    exact = p @ m[:, :3].T + m[:, 3]
    scale = np.abs(p) @ np.abs(m[:, :3]).T + np.abs(m[:, 3])
    return exact, GAMMA4 * scale, scale


def rigid(rpy, t):
    """3x4 float32 [R | t] from roll / pitch / yaw (formed in float64, rounded once) and a translation."""
    r, p, y = (float(a) for a in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    rot = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                    [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                    [-sp, cp * sr, cp * cr]])
    return np.concatenate([rot, np.asarray(t, np.float64).reshape(3, 1)], 1).astype(F)


def pack_pointcloud2(xyz, point_step, off_x, off_y, off_z, fill=0xA5, off_label=None, labels=None):
    """Tightly packed little-endian PointCloud2 rows; the bytes no field covers hold `fill`."""
    p = np.ascontiguousarray(xyz, dtype="<f4").reshape(-1, 3)
    buf = np.full((len(p), point_step), fill, np.uint8)
    for k, off in enumerate((off_x, off_y, off_z)):
        buf[:, off:off + 4] = p[:, k:k + 1].copy().view(np.uint8)
    if off_label is not None:
        buf[:, off_label:off_label + 4] = np.ascontiguousarray(labels, dtype="<u4").reshape(-1, 1).view(np.uint8)
    return buf.tobytes()
