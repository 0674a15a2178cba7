"""numpy reference of the occupied-bin statistic (mcl_3dl_amd/csrc/particle_bins.h): every step is a single IEEE
operation — float32 for the key arithmetic, float64 for the sector test, over the table the library itself hands out — so keys,
counts, leaders, occupied and occupied_alive are expected bit for bit; masses are math.fsum's, the exactly rounded sums."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
MAX_KEYS = 0xfffffffe


class BinsTooSmall(ValueError):
    pass


def finite_rows(pos):
    return np.isfinite(np.asarray(pos, F32)).all(axis=1)


def make_grid(pos, bin_xyz, yaw_bins):
    """(inv float32[3], min_b int64[3], div int64[3]) of the finite positions, or None when there is none."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    ok = finite_rows(pos)
    if not ok.any():
        return None
    inv = F32(1.0) / np.asarray(bin_xyz, F32)
    lo, hi = pos[ok].min(axis=0), pos[ok].max(axis=0)
    flo, fhi = np.floor(lo * inv), np.floor(hi * inv)
    if not (np.abs(flo) < 2.0 ** 31).all() or not (np.abs(fhi) < 2.0 ** 31).all():
        raise BinsTooSmall()
    min_b, max_b = flo.astype(np.int64), fhi.astype(np.int64)
    div = max_b - min_b + 1
    if (div > 2 ** 31 - 1).any() or int(div[0]) * int(div[1]) * int(div[2]) * int(yaw_bins) > MAX_KEYS:
        raise BinsTooSmall()
    return inv, min_b, div


def axis_bins(pos, inv, min_b):
    """i_a = (int)(floorf(p_a * inv_a) - (float)min_b_a), (n, 3) int32; rows with a non-finite position hold garbage."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = pos * inv                      # float32 product
        rel = np.floor(scaled) - min_b.astype(F32)
        rel = np.where(np.isfinite(rel), rel, F32(0))
        return rel.astype(np.int32)


def yaw_terms(rot):
    """t0, t1 of Quat::getRPY: float products and sums, the tails in double, rounded to float."""
    x, y, z, w = (np.asarray(rot, F32).reshape(-1, 4)[:, k] for k in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        ysq = y * y
        s0 = ysq + z * z
        s1 = x * y + w * z
        t0 = (F64(-2.0) * s0.astype(F64) + F64(1.0)).astype(F32)
        t1 = (F64(2.0) * s1.astype(F64)).astype(F32)
    return t0, t1


def sectors(t0, t1, table):
    """The first j with c_j t1 - s_j t0 >= 0 and c_{j+1} t1 - s_{j+1} t0 < 0 (double, unfused); 0 when none qualifies."""
    table = np.asarray(table, F64).reshape(-1, 2)
    if len(table) == 1:
        return np.zeros(len(t0), np.int32)
    a, b = t1.astype(F64)[:, None], t0.astype(F64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        side = table[None, :, 0] * a - table[None, :, 1] * b
    hit = (side >= 0) & (np.roll(side, -1, axis=1) < 0)
    return np.where(hit.any(axis=1), hit.argmax(axis=1), 0).astype(np.int32)


def keys(rows7, grid, table):
    """uint32 keys of (n, 7) rows {position, quaternion xyzw}; non-finite positions get the key above all others."""
    rows7 = np.asarray(rows7, F32).reshape(-1, 7)
    inv, min_b, div = grid
    yb = len(np.asarray(table).reshape(-1, 2))
    i = axis_bins(rows7[:, :3], inv, min_b).astype(np.uint32).astype(np.uint64)
    sec = sectors(*yaw_terms(rows7[:, 3:7]), table).astype(np.uint64)
    d = div.astype(np.uint64)
    key = (((i[:, 2] * d[1] + i[:, 1]) * d[0] + i[:, 0]) * np.uint64(yb) + sec) & np.uint64(0xffffffff)
    nonfinite = np.uint64(int(div[0]) * int(div[1]) * int(div[2]) * yb)
    return np.where(finite_rows(rows7[:, :3]), key, nonfinite).astype(np.uint32)


def key_parts(key, grid, yaw_bins):
    """key -> absolute {ix, iy, iz, sector}."""
    _, min_b, div = grid
    cell, sector = divmod(int(key), int(yaw_bins))
    return [cell % int(div[0]) + int(min_b[0]), cell // int(div[0]) % int(div[1]) + int(min_b[1]),
            cell // int(div[0]) // int(div[1]) + int(min_b[2]), sector]


def leader_of(idx, w):
    """The particle with the largest weight, the lowest index on a tie; a NaN weight leads only where every weight is one."""
    real = ~np.isnan(w)
    if not real.any():
        return int(idx[0])
    return int(idx[real][np.argmax(w[real])])


def bins(rows7, weights, bin_xyz, yaw_bins, table, top_k=0):
    """The whole statistic: dict(occupied, occupied_alive, nonfinite, bins = {key: (count, mass, leader, abs_mass)}, top = [(bin4,
    mass, count, leader)], grid). abs_mass = fsum(|w|) of the bin, for error bounds."""
    rows7 = np.asarray(rows7, F32).reshape(-1, 7)
    weights = np.asarray(weights, F32).reshape(-1)
    grid = make_grid(rows7[:, :3], bin_xyz, yaw_bins)
    ok = finite_rows(rows7[:, :3])
    out = dict(occupied=0, occupied_alive=0, nonfinite=int((~ok).sum()), bins={}, top=[], grid=grid, keys=None)
    if grid is None:
        return out
    key = keys(rows7, grid, table)
    out["keys"] = key
    idx = np.nonzero(ok)[0]
    order = idx[np.argsort(key[idx], kind="stable")]
    sorted_keys = key[order]
    starts = np.concatenate([[0], np.nonzero(sorted_keys[1:] != sorted_keys[:-1])[0] + 1, [len(order)]])
    for s, e in zip(starts[:-1], starts[1:]):
        members = order[s:e]
        w = weights[members]
        w64 = [float(v) for v in w]
        out["bins"][int(sorted_keys[s])] = (int(e - s), math.fsum(w64), leader_of(members, w), math.fsum(abs(v) for v in w64))
    out["occupied"] = len(out["bins"])
    out["occupied_alive"] = sum(1 for b in out["bins"].values() if b[1] > 0)
    ranked = sorted((k for k, b in out["bins"].items() if not math.isnan(b[1])), key=lambda k: (-out["bins"][k][1], k))
    out["top"] = [(key_parts(k, grid, yaw_bins),) + out["bins"][k][1:2] + out["bins"][k][0:1] + out["bins"][k][2:3]
                  for k in ranked[:top_k]]
    return out


def kld_bound_exact(k, epsilon, z, digits=50):
    """Fox's bound evaluated in decimal arithmetic at `digits` digits: (value before ceil as Decimal, ceil as int)."""
    from decimal import Decimal, getcontext, ROUND_CEILING
    getcontext().prec = digits
    k1 = Decimal(k - 1)
    b = Decimal(2) / (Decimal(9) * k1)
    x = Decimal(1) - b + b.sqrt() * Decimal(float(z))   # (the doubles' exact values)
    value = k1 / (Decimal(2) * Decimal(float(epsilon))) * x * x * x
    return value, int(value.to_integral_value(rounding=ROUND_CEILING))
