"""Term vectors for the reference's float recurrence s = fl(s + t) (likelihood.cpp:120-134, pf.h:255-260) at the inputs where
mcl_3dl_amd/csrc/float_chain.h:seq_sum_wave leaves its shortcut: shared by the CPU replay (tests/cpp/float_chain_emul.cpp through
tests/test_float_chain_cpu.py, which also states what every case exercises) and by the kernels that run the wavefront form on
the device (tests/test_gpu_float_chain_adversarial.py). Seeded, pure numpy float32; the expected sum is prefix_loop(t)[-1].

A case is (name, t). Where seq_sum_wave's layout matters: the first 256 terms are added serially (CHAIN_HEAD4 quads), a pass
behind them takes 512 terms (lane L of 64 holds the eight terms 8 L .. 8 L + 7 of the pass), pf_fused_kernel and
update_small_kernel hand it up to 1024 terms as one row, pf_strict_sum_kernel rows of 4096 with the sum carried between them."""
import numpy as np

F = np.float32
HEAD = 256       # terms of the serial head
PASS = 512       # terms of one wavefront pass
CHUNK = 4096     # terms pf_strict_sum_kernel stages at a time
FUSED_MAX = 1024
# the head alone, one quad and one term past it; one full pass behind the head; the fused limit; the strict-sum chunk with its
# carried sum on either side; several chunks
SIZES = (1, 255, 256, 257, 260, 261, 768, 769, 1000, 1024, 1025, 4095, 4096, 4097, 8197, 20000)
SPECIAL_VALUES = (("nan", F(np.nan)), ("inf", F(np.inf)), ("neg", F(-0.125)), ("negzero", F(-0.0)), ("huge", F(3e38)),
                  ("denormal", F(1e-45)))
EVERY_LANE_SIZES = (1000, CHUNK + 1000)


def prefix_loop(terms):
    """acc = 0; acc += t in float32, every prefix (np.add.accumulate on float32 is this loop, started at +0 as in C: 0 + -0 is
    +0; NaN and inf propagate)."""
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([[F(0)], np.asarray(terms, F)]), dtype=F)[1:]


def serial_sum(terms):
    return prefix_loop(terms)[-1]


def same_bits(a, b):
    """Equal as uint32 patterns, any NaN equal to any NaN."""
    a, b = np.atleast_1d(np.asarray(a, F)), np.atleast_1d(np.asarray(b, F))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def _rng(family, n):
    return np.random.default_rng([family, n])


def weights(n):
    """(0.5 + U) * 30 / n: un-normalised weights of similar size (pf.h:255-260) — long runs of clean passes."""
    u = _rng(1, n).random(n, dtype=F)
    return ((F(0.5) + u) * F(30.0) / F(n)).astype(F)


def ties(n):
    """Every third term or so, once the sum has passed 4, is an odd multiple of half an ulp of the running sum's binade: the
    rounding of s + t then hangs on the parity of s (family 2 of the CPU replay's own run)."""
    rng = _rng(2, n)
    u = rng.random(n, dtype=F)
    pick = rng.integers(0, 3, n)
    odd = (2 * rng.integers(0, 2000, n) + 1).astype(F)
    t = np.empty(n, F)
    s = F(0)
    for i in range(n):
        if s > 4.0 and pick[i] == 0:
            half_ulp = (np.array([s], F).view(np.uint32) & np.uint32(0x7f800000)) - np.uint32(24 << 23)
            t[i] = half_ulp.view(F)[0] * odd[i]
        else:
            t[i] = u[i]
        s = F(s + t[i])
    return t


def wild(n):
    """ldexp(U, e), e in [-45, 15): binade crossings everywhere, terms that are huge against the sum; zeros; denormals 2^-140
    (family 3 of the CPU replay's own run)."""
    rng = _rng(3, n)
    t = np.ldexp(rng.random(n, dtype=F), rng.integers(-45, 15, n).astype(np.int32)).astype(F)
    t[rng.integers(0, 11, n) == 0] = F(0)
    t[rng.integers(0, 997, n) == 0] = np.ldexp(F(1), -140)
    return t


def tie_constant(n, bits=9):
    """1 / n with its low `bits` mantissa bits set to 100...0: added n times, a rounding tie at every step of one binade."""
    u = np.array([F(1.0) / F(n)], F).view(np.uint32)
    u = (u & ~np.uint32((1 << bits) - 1)) | np.uint32(1 << (bits - 1))
    return u.view(F)[0]


def equal(n):
    return np.full(n, tie_constant(n, 9), F)


def special_positions(n):
    """The first term, the last of the head, the first of the first pass, lane 63 of the first pass, the middle, the last."""
    return sorted({p for p in (0, HEAD - 1, HEAD, HEAD + 8 * 63 + 3, n // 2, n - 1) if p < n})


def specials(n):
    """The weights family with ONE term replaced: [(name, t)]."""
    base = weights(n)
    out = []
    for tag, v in SPECIAL_VALUES:
        for pos in special_positions(n):
            t = base.copy()
            t[pos] = v
            out.append(("%s@%d" % (tag, pos), t))
    return out


def every_lane(n, lane):
    """A -0.0 in lane `lane` of a pass that would otherwise be clean (it fails chain_classify's one unsigned compare, takes the serial
    path and changes no value), and another in lane 63 - lane of the pass that restarts behind it.

    The weights family itself cannot place a lane: its sum triples during the first pass, so a binade's edge comes first. Here
    the sum is pinned to [32, 64) by a leading 32 and the other terms are weights rounded to that binade's ulp, 2^-18 — no
    rounding tie, no crossing (32 + 1.5 * 30 stays below 64), every term below 2^4 — so that the -0.0 is the FIRST trouble of
    its pass. n = 1000: one row (pf_fused_kernel, update_small_kernel). n = 4096 + 1000: the second row of
    pf_strict_sum_kernel, behind a carried sum and a restarted head (the family's terms add up to about 30 whatever n is, so
    the sum stays in [32, 64) there too)."""
    assert n in EVERY_LANE_SIZES and 0 <= lane < 64
    t = np.ldexp(np.rint(np.ldexp(weights(n), 18)), -18).astype(F)
    t[0] = F(32.0)
    row = n - 1000
    first = row + HEAD + 8 * lane            # this lane's eight terms of the row's first pass
    t[first + lane % 8] = F(-0.0)
    second = first + 8 + 8 * (63 - lane)     # the next pass starts behind those eight terms
    t[second + (lane + 3) % 8] = F(-0.0)
    return t


FAMILIES = ("weights", "ties", "wild", "equal", "specials", "every_lane")


def family_cases(family, n):
    """[(name, t)] of one family at one size (every_lane: n in EVERY_LANE_SIZES, one case per lane)."""
    if family == "specials":
        return [("specials/%d/%s" % (n, tag), t) for tag, t in specials(n)]
    if family == "every_lane":
        return [("every_lane/%d/%d" % (n, lane), every_lane(n, lane)) for lane in range(64)]
    return [("%s/%d" % (family, n), {"weights": weights, "ties": ties, "wild": wild, "equal": equal}[family](n))]


def all_cases():
    out = []
    for family in FAMILIES:
        for n in (EVERY_LANE_SIZES if family == "every_lane" else SIZES):
            out += family_cases(family, n)
    return out


def write_cases(path, cases):
    """The file tests/cpp/float_chain_emul.cpp reads: int32 count, then per case int32 n and n float32 (little endian)."""
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], "<i4").tobytes())
        for _, t in cases:
            t = np.ascontiguousarray(t, "<f4")
            f.write(np.array([len(t)], "<i4").tobytes())
            f.write(t.tobytes())
