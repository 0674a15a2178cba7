"""The cases of tests/test_gpu_lik_exact.py — the fp64-tree likelihood sums against exact sums of the reference's terms
(tests/lik_terms_ref.py) — built here so that tests/test_lik_terms_cpu.py checks their preconditions without a GPU: the
restatement equals the oracle on the very particles the GPU test looks at, and the SHARPNESS condition holds on them (at most
0.2 % of a particle's non-zero terms are <= one float32 ulp of its exact sum, so a bound of half an ulp sees practically every
lost, doubled or mis-matched term; at least 8 matched points).

Every case is make_scene(n=91, ...), a 50 k-point map, seeded. The shapes are the smallest at which the code can go wrong:
a tile is 256 points, a particle group G of 4 / 8 / 16 / 32, blockIdx -> (tile, group) walks the tiles = x (mod 8), and
lik_finalize_kernel has 8 slices over the tiles and 32 particles per work-group (likelihood_kernels.h, host_measure.h)."""
import functools
from dataclasses import dataclass

import numpy as np

import lik_terms_ref as lt
from mcl_3dl_amd.synthetic import make_scene

F = np.float32
LATTICE, JITTER = 0.0, 0.045          # map_jitter: the lattice; centroids displaced in their voxels (overflow records, deferred rounds)
UNIT, TALL = (1.0, 1.0, 1.0), (1.0, 1.0, 5.0)  # dist_weight
MAX_CHECKED = 48
SMALL_SHARE_CAP = 0.002
MIN_MATCHED = 8
DEFAULTS = dict(strict_order=2, lik_group=0, lik_tiled=1)  # what a case's options are set back to


@dataclass(frozen=True)
class Case:
    id: str
    n_p: int
    n_s: int
    jitter: float
    dist_weight: tuple
    flat: float
    options: tuple = ()       # ((name, value), ...) on top of the defaults
    entry: str = "batch"      # batch: measure_batch; update: measure_update from host arrays; group / group-update: the same two
                              # through three contexts on one device
    n_b: int = 0
    seed: int = 5
    min_matched: int = MIN_MATCHED
    route: str = "tiled/fp64/finalize"  # kernel / sum / who adds the tiles: what the case is there for, == route_of(case)
                                        # (tests/test_lik_terms_cpu.py; the GPU test asserts the option defaults behind it)

    @property
    def tiled(self):
        return self.route.startswith("tiled")

    @property
    def opts(self):
        return dict(self.options)

    @property
    def params(self):
        return lt.params(match_dist_flat=self.flat)

    def scene(self):
        return scene(self.n_p, self.n_s, self.n_b, self.jitter, self.seed)

    def group_size(self):
        """host_measure.h:plan_group_size — the particles per work-group of the tiled kernel."""
        g = self.opts.get("lik_group", 0)
        if g:
            return g
        n_tiles = (self.n_s + 255) // 256
        for gg in (16, 8, 4):
            if n_tiles * ((self.n_p + gg - 1) // gg) >= 2048:
                return gg
        return 4

    def particles_per_work_group(self):
        if self.tiled:
            return self.group_size()
        if self.route.startswith("small"):  # likelihood_small_kernel: 256 / W particles per work-group, W = 2^k >= n_s
            return 256 >> max(self.n_s - 1, 0).bit_length()
        return 1

    def shards(self):
        """[begin, end) of the particles every launch of the case covers."""
        if not self.entry.startswith("group"):
            return [(0, self.n_p)]
        from mcl_3dl_amd import capi
        out = []
        for r in range(3):
            b, c = capi.group_shard(self.n_p, 3, r)
            out.append((b, b + c))
        return out

    def checked(self):
        """The particles to check: at most 48, never fewer than min(n_p, 24); per launch the whole first group, the whole last
        (ragged) one, either side of the 32-particle finalize boundaries up to 64, and an even spread over the rest."""
        sh = self.shards()
        wg = 64 if self.route.endswith("pf-tail") else None  # lik_pf_partial_kernel: 64 particles per work-group
        idx = np.concatenate([lo + checked_of(hi - lo, self.particles_per_work_group(), MAX_CHECKED // len(sh), wg) for lo, hi in sh])
        assert min(self.n_p, 24) <= len(idx) <= MAX_CHECKED and len(np.unique(idx)) == len(idx)
        return idx


# ---- the route of a case: host_measure.h and host_pf.h restated over the option defaults ------------------------------------------
# (the GPU test asserts that the engine's options hold these values; the constants are host_options.h's and host_measure.h's)
OPTION_DEFAULTS = dict(strict_order=2, lik_tiled=1, lik_tiled_min=1024, lik_group=0, lik_small=1, lik_index=2, strict_exact_max=4096,
                       strict_auto_min=28147, strict_chunk=0, update_small=1, update_small_max=512, pf_fused=1)
LIK_ROW_MAX, STRICT_ROWS_MAX_PARTICLES, LIK_WIDE_MAX_PARTICLES, PF_FUSED_MAX_PARTICLES = 12288, 2048, 512, 1024


def route_of(case):
    """"<kernel>/<sum>[/<who adds the tiles>]" as lik_mode, lik_small_applies, lik_particle_block, launch_update_small, pf_form /
    pf_takes_tiles and the device group's update decide it for the case's shape, entry point and options."""
    o = dict(OPTION_DEFAULTS, **case.opts)
    n_s, strict = case.n_s, o["strict_order"]
    assert strict in (0, 2) and o["lik_index"] == 2
    n_p = min(hi - lo for lo, hi in case.shards())  # (a rank decides for its own shard; the shards here all decide alike)
    assert len({route_np(o, hi - lo, n_s, case) for lo, hi in case.shards()}) == 1
    return route_np(o, n_p, n_s, case)


def route_np(o, n_p, n_s, case):
    strict = o["strict_order"]
    by_size = bool(o["lik_tiled"]) and n_p >= 4 and (n_s >= o["lik_tiled_min"] or (n_p >= 256 and 4 * n_s >= 3 * o["lik_tiled_min"]))
    exact = strict == 2 and (n_s <= o["strict_exact_max"] or n_s >= o["strict_auto_min"])
    rows_fit = n_s <= LIK_ROW_MAX and o["strict_chunk"] == 0
    if not exact:
        tiled, rows, replay = by_size, (not by_size) and strict == 2 and rows_fit, False
    elif rows_fit and (not by_size or n_p < STRICT_ROWS_MAX_PARTICLES):
        tiled, rows, replay = False, True, False
    else:
        tiled, rows, replay = True, False, True
    total = "rows" if rows else ("replay" if replay else "fp64")
    if tiled:
        if case.entry == "group-update":     # a rank's first pf::measure kernel always takes the tiles (pf_tiles_fit)
            tail = "pf-tail"
        elif case.entry == "update":         # pf_takes_tiles: the split form with the fp64 tree over the weights
            fused = bool(o["pf_fused"]) and n_p <= PF_FUSED_MAX_PARTICLES
            float_w = strict == 2 and n_p <= PF_FUSED_MAX_PARTICLES
            tail = "pf-tail" if not fused and not float_w and n_p <= 1024 * 256 else "finalize"
        else:
            tail = "finalize"
        return "tiled/%s/%s" % (total, tail)
    if n_s <= 32 and n_p >= 256 and o["lik_small"]:
        return "small/%s" % total
    block = 64 if n_s <= 128 else (1024 if n_p <= LIK_WIDE_MAX_PARTICLES and n_s > 512 else 256)
    one = case.entry == "update" and o["update_small"] and n_p <= o["update_small_max"] and case.n_b <= 256
    return "%s%d/%s" % ("one-launch" if one else "particle", block, total)


def checked_of(n_p, g, cap, wg=None):
    """g: particles per work-group of the kernel that forms the terms; wg: of the one that adds the tiles, where that is not
    lik_finalize_kernel's 32 — its last work-group is checked whole where the cap leaves room for it."""
    if n_p <= cap:
        return np.arange(n_p)
    last = (n_p - 1) // g * g
    must = set(range(min(g, n_p))) | set(range(last, n_p)) | {i for i in (31, 32, 63, 64) if i < n_p}
    if wg and len(must | set(range((n_p - 1) // wg * wg, n_p))) <= cap:
        must |= set(range((n_p - 1) // wg * wg, n_p))
    must = sorted(must)
    assert len(must) <= cap, (n_p, g, cap)
    room = cap - len(must)
    rest = np.setdiff1d(np.arange(n_p), must)
    spread = rest[np.linspace(0, len(rest) - 1, room).round().astype(np.int64)] if room else np.zeros(0, np.int64)
    return np.unique(np.concatenate([np.asarray(must, np.int64), spread]))


@functools.lru_cache(maxsize=None)
def scene(n_p, n_s, n_b, jitter, seed):
    return make_scene(n=91, n_p=n_p, n_s=n_s, n_b=n_b, seed=seed, map_jitter=jitter)


@functools.lru_cache(maxsize=None)
def _oracle(kind, jitter, map_seed, dist_weight, flat):
    sc = scene(1, 1, 0, jitter, map_seed)  # (the map depends on the jitter and, with a jitter, on the seed alone)
    return lt.make_oracle(kind, sc.map_xyz, sc.map_label, dist_weight, lt.params(match_dist_flat=flat))


def oracle(kind, case):
    return _oracle(kind, case.jitter, case.seed if case.jitter else 0, case.dist_weight, case.flat)


_listings = {}


def listing(kind, case, particle):
    """lik_terms_ref.particle_terms of one particle of the case; computed once per (scene, metric, flat, particle)."""
    key = (kind, case.n_p, case.n_s, case.n_b, case.jitter, case.seed, case.dist_weight, case.flat, int(particle))
    if key not in _listings:
        sc = case.scene()
        _listings[key] = lt.particle_terms(oracle(kind, case), sc.poses[particle], sc.scan_lik, case.params)
    return _listings[key]


def check_sharpness(case, lst, particle):
    share = lt.small_term_share(lst)
    assert lst.count >= case.min_matched, "%s: particle %d matches %d points only" % (case.id, particle, lst.count)
    assert share <= SMALL_SHARE_CAP, "%s: %.3g of particle %d's terms are below one ulp of its sum" % (case.id, share, particle)
    return share


# ---- the tiled kernel in the default mode (strict_order 2), 4097 .. 28 146 points ---------------------------------------------------
def _c(name, n_p, n_s, jitter, dw, flat, **kw):
    opts = tuple(sorted(kw.pop("options", {}).items()))
    return Case("%s-%dx%d-%s-%s-flat%g%s" % (name, n_p, n_s, "jitter" if jitter else "lattice", "tall" if dw == TALL else "unit", flat,
                                              "".join("-%s%d" % kv for kv in opts)), n_p, n_s, jitter, dw, flat, options=opts, **kw)


TILED = [
    # fewest particles that tile; 17 tiles, the last holds one point
    _c("tiled", 4, 4097, LATTICE, UNIT, 0.05), _c("tiled", 4, 4097, JITTER, TALL, 0.0),
    # 17 full tiles (2 x 8 + 1 over the finalize slices); the last group is ragged for every G
    _c("tiled", 37, 4352, LATTICE, TALL, 0.18), _c("tiled", 37, 4352, JITTER, UNIT, 0.05, options=dict(lik_group=32)),
    # 24 tiles, the last one point short; every group size
    _c("tiled", 300, 6143, LATTICE, UNIT, 0.05), _c("tiled", 300, 6143, JITTER, TALL, 0.0, options=dict(lik_group=4)),
    _c("tiled", 300, 6143, LATTICE, UNIT, 0.05, options=dict(lik_group=8)), _c("tiled", 300, 6143, JITTER, TALL, 0.0, options=dict(lik_group=16)),
    _c("tiled", 300, 6143, LATTICE, UNIT, 0.05, options=dict(lik_group=32)),
    # 33 tiles, the last holds one point; more than 256 groups at G = 4
    _c("tiled", 1100, 8193, LATTICE, TALL, 0.0, options=dict(lik_group=4)), _c("tiled", 1100, 8193, JITTER, UNIT, 0.18),
    # the benchmark's scan; an odd particle count across the finalize work-groups of 32
    _c("tiled", 4099, 16384, LATTICE, UNIT, 0.05), _c("tiled", 4099, 16384, JITTER, TALL, 0.18),
    # the last size of the fp64 default: 110 tiles, the last holds 242 points
    _c("tiled", 2051, 28146, LATTICE, TALL, 0.05), _c("tiled", 2051, 28146, JITTER, UNIT, 0.0),
]
BENCH_SCAN = TILED[11]

# ---- strict_order 0: everything the tiled kernel leaves -----------------------------------------------------------------------------
S0 = dict(strict_order=0)
# (a scan of 1 or 8 points cannot be asked for 8 matches of every particle: the seed of the 8-point scan is the best of 25 tried,
# at least 4 matches; the 32-point scan's seed restores the 8)
FP64_ELSEWHERE = [
    _c("one", 1, 1, LATTICE, UNIT, 0.05, options=S0, route="particle64/fp64", min_matched=1),
    _c("block64", 5, 33, JITTER, TALL, 0.0, options=S0, route="particle64/fp64"),
    _c("c1", 64, 1000, LATTICE, TALL, 0.05, options=S0, route="particle1024/fp64", seed=6),  # (seed 5: one of ~270 terms below an ulp, 0.37 %)
    _c("c1-one-launch", 64, 1000, JITTER, UNIT, 0.18, options=S0, route="one-launch1024/fp64", entry="update"),
    _c("block256", 600, 300, LATTICE, UNIT, 0.18, options=S0, route="particle256/fp64"),  # (129 .. 512 points: the 256-thread work-group)
    _c("small", 300, 8, LATTICE, UNIT, 0.0, options=S0, route="small/fp64", seed=23, min_matched=4),
    _c("small", 300, 32, JITTER, TALL, 0.05, options=S0, route="small/fp64", seed=14),
    # (from 1024 points on 64 particles tile: the 1024-thread work-group of the per-particle kernel gets a scan of 3000 with lik_tiled 0)
    _c("block1024", 64, 3000, JITTER, UNIT, 0.05, options=dict(strict_order=0, lik_tiled=0), route="particle1024/fp64"),
    _c("never-tiles", 3, 16384, LATTICE, TALL, 0.18, options=S0, route="particle1024/fp64"),
    _c("three-quarter", 700, 1000, JITTER, TALL, 0.0, options=S0),
]

# ---- entry points beyond measure_batch ------------------------------------------------------------------------------------------------
N_BEAM = 64
ENTRIES = [
    _c("merged-beam", 300, 6143, LATTICE, UNIT, 0.05, n_b=N_BEAM),            # the likelihood + beam launch carries the tiles
    # measure_update from host arrays. Up to 1024 particles pf::measure is the fused kernel and lik_finalize_kernel adds the tiles ...
    _c("update", 300, 6143, JITTER, TALL, 0.0, entry="update"),
    # ... beyond, lik_pf_partial_kernel does (pf_takes_tiles) — the tail of every C2 .. C4 update: 64 particles per work-group (the last
    # one holds 12), two slices per wavefront side by side while `tl + 4 < n_tiles`, then one more tile. 29 tiles: tiles 25 .. 27 are
    # that last trip's, the one-point tile 28 is a second slice's
    _c("update-tail", 1100, 7169, JITTER, UNIT, 0.18, entry="update", route="tiled/fp64/pf-tail"),
    # 24 tiles, the last one point short: no last trip; 2051 particles: a last work-group of 3
    _c("update-tail", 2051, 6143, LATTICE, TALL, 0.05, entry="update", route="tiled/fp64/pf-tail"),
    _c("group", 300, 6143, LATTICE, UNIT, 0.05, entry="group", options=dict(lik_group=8)),  # every rank tiles its own ragged shard
    # a rank's update always leaves its tiles to lik_pf_partial_kernel: 100 particles, a work-group of 64 and one of 36
    _c("group-update", 300, 6143, LATTICE, UNIT, 0.05, entry="group-update", options=dict(lik_group=8), route="tiled/fp64/pf-tail"),
]

CASES = TILED + FP64_ELSEWHERE + ENTRIES
assert len({c.id for c in CASES}) == len(CASES)

# ---- the window of the fp64 default from outside: the reference's float recurrence, bit for bit ---------------------------------
WINDOW = [_c("near-edge", 300, 4096, LATTICE, UNIT, 0.05, route="particle1024/rows"),
          _c("far-edge", 2051, 28147, JITTER, TALL, 0.05, route="tiled/replay/finalize")]
