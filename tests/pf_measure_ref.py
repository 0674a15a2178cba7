"""pf::ParticleFilter::measure (include/mcl_3dl/pf.h:252-279) with the lambda's product (src/mcl_3dl.cpp:407-424), restated once in
float32 for the tests: what mcl_3dl_amd/csrc/pf_sums.h and the four kernels that call it must compute, bit for bit, wherever
they add the weights in the reference's order (float_chain.h). tests/test_motion_cpu.py checks the `w * lik` case of it against
the reference's own weights and restore flags (tests/golden/motion.npz)."""
import math

import numpy as np

from float_chain_cases import serial_sum

F = np.float32


def pf_weight(w, lik, beam=None, extra=None):
    """l = 1; l *= beam; l *= lik; l = l * extra; wn = w * l — every product rounded to float; a factor the update does not have
    is 1 (x * 1 is x in every bit)."""
    w, lik = np.asarray(w, F), np.asarray(lik, F)
    with np.errstate(all="ignore"):
        l = np.ones(len(w), F)
        l = (l * (F(1) if beam is None else np.asarray(beam, F))).astype(F)
        l = (l * lik).astype(F)
        l = (l * (F(1) if extra is None else np.asarray(extra, F))).astype(F)
        return (w * l).astype(F)


def measure(w, lik, beam=None, extra=None):
    """dict(wn, sum, restored, weights): sum = the serial float loop over wn in particle order; restore (weights untouched) unless
    sum > 0 — NaN, a negative sum and 0 restore, +inf does not; otherwise wn / sum, each quotient rounded to float."""
    w = np.asarray(w, F)
    wn = pf_weight(w, lik, beam, extra)
    s = serial_sum(wn)
    restored = not s > 0.0
    with np.errstate(all="ignore"):
        weights = w.copy() if restored else (wn / s).astype(F)
    return dict(wn=wn, sum=s, restored=restored, weights=weights)


def pf_measure(w, lik, beam=None, extra=None):
    """(weights, restored)."""
    m = measure(w, lik, beam, extra)
    return m["weights"], m["restored"]


def entropy(wn, s):
    """(H, bound) of an alive update with a finite sum: H = ln S - T / S with S the sum as a double and T = sum wn ln wn over
    wn > 0 in float64 (math.fsum) — what -sum (wn / S) ln (wn / S) is, 0 ln 0 = 0. bound: the float rounding of the result,
    2^-23 |H|, plus 2^-36 (|ln S| + sum |wn ln wn| / S) for an fp64 tree over up to 20 000 terms and the log's own error."""
    S = float(s)
    x = np.asarray(wn, np.float64)
    x = x[x > 0]
    terms = x * np.log(x)
    T, A = math.fsum(terms), math.fsum(np.abs(terms))
    H = math.log(S) - T / S
    return H, 2.0 ** -23 * abs(H) + 2.0 ** -36 * (abs(math.log(S)) + A / S)
