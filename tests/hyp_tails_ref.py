"""The reference of the two-tailed hypergeometric test (hypergeom_tails = 'attribute_sign'): the exact lower tail as a Fraction
beside tests/hyp_exact.py's upper tail, the NumPy restatement of NES / binarisation / counts for the three signs, and the same
decision made on the exact rationals (what the GPU tests hold nes_binary to).  Nothing here touches a device."""
from fractions import Fraction

import numpy as np

import hyp_exact as hx

SIGNS = ('highest', 'lowest', 'both')
BAND = Fraction(1, 10 ** 6)                                     # cells this close (relative) to a threshold are left out


def exact_lower_tail(pop, K, n, x):
    """P[H <= x] for H ~ Hypergeom(pop, K, n) as a Fraction: 0 below the support, 1 at or above its top (scipy's cdf)."""
    return 1 - hx.exact_tail(pop, K, n, x + 1)


def mirror(b):
    """The 0/1 matrix with zeros and ones swapped, NaN kept: K -> pop - K and x -> n - x for every cell."""
    return np.where(np.isnan(b), np.nan, 1.0 - b)


# ---- the NumPy restatement (safe.py:546-554 without the 1 / P substitution, 608, 468-472) ---------------------------------

def nes(p_pos, p_neg, sign):
    with np.errstate(divide='ignore', invalid='ignore'):
        ep, en = -np.log10(p_pos), -np.log10(p_neg)
        return {'highest': ep, 'lowest': en, 'both': ep - en}[sign]


def nes_binary(nes_values, threshold):
    with np.errstate(invalid='ignore'):
        out = (np.abs(nes_values) > -np.log10(threshold)).astype(np.float64)
    out[np.isnan(nes_values)] = 0
    return out


def outputs(p_pos, p_neg, sign, threshold):
    """(nes, nes_binary, num_neighborhoods_enriched)."""
    v = nes(np.asarray(p_pos, dtype=np.float64), np.asarray(p_neg, dtype=np.float64), sign)
    nb = nes_binary(v, threshold)
    return v, nb, nb.sum(axis=0)


# ---- the same decision on exact rationals ----------------------------------------------------------------------------------

def exact_nes(e_pos, e_neg, sign):
    """-log10 of the exact tails (120-bit logarithms), combined as the sign says; +-inf where a tail is 0."""
    if sign == 'highest':
        return hx.neg_log10(e_pos)
    if sign == 'lowest':
        return hx.neg_log10(e_neg)
    return hx.neg_log10(e_pos) - hx.neg_log10(e_neg)            # (both tails 0 cannot happen: they sum to more than 1)


def exact_decision(e_pos, e_neg, sign, thr):
    """(enriched, left_out) for exact tails and an exact threshold `thr` (a Fraction).  One side: p < thr, cells within BAND
    of thr left out -- except p == thr exactly, which is kept and not enriched.  'both': |log10(p_neg / p_pos)| > -log10 thr,
    i.e. the ratio p_neg / p_pos above 1 / thr or below thr; cells whose ratio is within BAND of either are left out."""
    if sign in ('highest', 'lowest'):
        e = e_pos if sign == 'highest' else e_neg
        if e == thr:
            return False, False
        if abs(e - thr) <= thr * BAND:
            return False, True
        return e < thr, False
    if e_pos == 0 or e_neg == 0:
        return True, False                                      # nes = +-inf
    ratio = e_neg / e_pos
    for bound in (thr, 1 / thr):
        if abs(ratio - bound) <= bound * BAND:
            return False, True
    return (ratio < thr or ratio > 1 / thr), False
