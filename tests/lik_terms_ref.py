"""The terms of LidarMeasurementModelLikelihood::measure (src/lidar_measurement_model_likelihood.cpp:105-139), one particle at a
time, from the oracle's primitives and numpy float32, in the style of tests/moments_ref.py:

    q = o.transform(pose7, scan)                 State6DOF::transform (:121-122)
    found, idx, sq = o.radius_search(q, r)       ChunkedKdtree::radiusSearch (:126; the dist_weight is applied inside)
    d    = sqrt_f32(sq)                          where found only: sq says nothing elsewhere
    dist = f32(r) - max(d, f32(flat))            :128
    keep = found & ~(dist < 0)                   :129
    term = f32(dist * f32(match_weight))         :132, one float product

The reference adds the terms in float, in scan order (score_like += term); np.cumsum(terms, dtype=float32)[-1] is therefore its
likelihood bit for bit and float32(count) / float32(n_s) its match ratio (:136) — tests/test_lik_terms_cpu.py pins both against
Oracle.likelihood_measure. Every operation above is correctly rounded (- max * sqrt), so numpy float32 gives the reference's bits.

The engine's fp64 tree (likelihood_kernels.h: likelihood_tiled_body + lik_finalize_kernel / lik_pf_partial_kernel, lik_particle,
likelihood_small_kernel without rows) forms the same float terms and ADDS them in double, in some tree, then narrows the sum to
float once. Its reference is so the EXACT sum of the terms (math.fsum), and the only room it has is the rounding of its own adds:

  bound(n, sum_abs) = n * 2^-53 * sum |t|

Derivation. A tree that adds n numbers does n - 1 additions; an addition with a zero operand is exact, so only the non-zero
terms count (n = the matched count is an upper bound of them; unmatched points hold +0). Each addition rounds its result by at
most u = 2^-53 relative, so a leaf passes through at most n - 1 factors (1 + delta), |delta| <= u, whatever the association:
|computed - exact| <= ((1 + u)^(n - 1) - 1) sum |t| <= (n - 1) u / (1 - (n - 1) u) sum |t| <= n u sum |t| as long as
n (n - 1) u <= 1, i.e. for every n below 9e7. (The terms are >= 0 here, so sum |t| is the exact sum itself.)

With float32 spacing 2^-11 at a sum of ~5000 and the bound at ~3e-9, the narrowed result is the correctly rounded exact sum
unless that sum lies within the bound of a rounding boundary — `within` allows exactly that."""
import math
from collections import namedtuple

import numpy as np

from oracle import pyoracle

F = np.float32
D = np.float64

Listing = namedtuple("Listing", "terms count exact sum_abs")


def params(match_dist_min=0.2, match_dist_flat=0.05, match_weight=5.0):
    return pyoracle.LikelihoodParams(match_dist_min=match_dist_min, match_dist_flat=match_dist_flat, match_weight=match_weight)


def make_oracle(kind, map_xyz, map_label, dist_weight, p):
    o = pyoracle.Oracle(kind)
    o.set_map(map_xyz, map_label, dist_weight=dist_weight)
    o.set_likelihood_params(p)
    return o


def particle_terms(o, pose7, scan, p):
    """The float32 terms of one particle in scan order ([n_s]; +0 where the point is unmatched), the matched count, the exact
    sum of the terms and sum |t|."""
    r, flat, mw = F(p.match_dist_min), F(p.match_dist_flat), F(p.match_weight)
    q = o.transform(pose7, scan)
    found, _, sq = o.radius_search(q, r)
    found = found != 0
    d = np.sqrt(np.where(found, sq, F(0)).astype(F)).astype(F)
    dist = (r - np.maximum(d, flat)).astype(F)
    keep = found & ~(dist < 0)
    terms = np.where(keep, (dist * mw).astype(F), F(0)).astype(F)
    wide = terms.astype(D)
    return Listing(terms, int(np.count_nonzero(keep)), math.fsum(wide.tolist()), math.fsum(np.abs(wide).tolist()))


def float_recurrence(terms):
    """score_like += term, float, in scan order: the reference's own likelihood."""
    return F(0) if len(terms) == 0 else np.cumsum(np.asarray(terms, F), dtype=F)[-1]


def ratio(count, n_s):
    """(float)num / n_s, :136."""
    return F(F(count) / F(n_s))


def bound(n_terms, sum_abs):
    """n * 2^-53 * sum |t|: the worst case of any association of n double additions of these floats (module docstring)."""
    return n_terms * 2.0 ** -53 * sum_abs


def tolerance(got, lst):
    """Half a float32 ulp for the single narrowing (at the exact sum or at the result, whichever binade is the wider) + bound."""
    e32 = F(lst.exact)
    return 0.5 * float(max(np.spacing(np.abs(e32)), np.spacing(np.abs(F(got))))) + bound(lst.count, lst.sum_abs)


def error_over_bound(got, lst):
    """|float64(got) - exact| over `tolerance`: <= 1 passes. (The correctly rounded exact sum, got == float32(exact), is within
    half its own spacing of the exact sum and so always passes; a result one float ulp to either side passes only where the
    exact sum lies within `bound` of the boundary between the two.)"""
    tol = tolerance(got, lst)
    err = abs(float(D(got)) - lst.exact)
    return err / tol if tol > 0 else math.inf


def small_term_share(lst):
    """The share of the non-zero terms that are <= one float32 ulp of the exact sum: those a lost or doubled term could hide
    behind (the sharpness condition of tests/lik_exact_cases.py)."""
    nz = lst.terms[lst.terms != 0]
    if len(nz) == 0:
        return 1.0
    return float(np.count_nonzero(nz.astype(D) <= float(np.spacing(F(lst.exact))))) / len(nz)
