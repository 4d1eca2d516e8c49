"""Designed inputs for the decision margins of the filtered matrix-core permutation tests, and their exact reference (CPU
only; the tests are tests/test_filter_margin_cases_cpu.py and tests/test_gpu_filter_margins.py).

The filtered forms (k_permtest_mfma_g, k_permtest_mfma_gz, the general kernel's FM = 2) decide a compare from the HIGH digits
(3-5) of the balanced base-256 fixed-point image alone when a margin says that the LOW digits (0-2) cannot change the answer.
A margin one unit too narrow misdecides only the compares that sit on its edge, so these inputs put a large share of ALL
compares within a factor four of each margin, with the low digits at their extremes:

* every value is an INTEGER stored as f64, every column holds an odd value and spans 32..46 bits -- so the column's unit is 1,
  the image is the value itself (q == b), the call runs six slices, hi = digits 3-5 and lo = digits 0-2 of the value;
* 'sum' families: b = offset + h 2^24 + lo with lo mostly -MF_LO_MAX or +127 x 65793 (the two ends of the low part);
* z-score families: b = 2^21 L (2^22 + e), L in {3, 5} -- neighborhoods of the same composition differ by ~e / 2^22 in their
  score, right where the single-precision decision's 2^-19 .. 2^-21 terms act; and b = h 2^24 + lo with h in 64..127, where
  the bound on the low parts is what the margins consist of.

Nothing here touches the library: the reference is integer arithmetic on the permutation tables it is handed."""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import safe_oracle as orc

MF_LO_MAX = 128 * 65793                 # -MF_LO_MAX = the most negative low part (digits 0-2 all -128)
LO_TOP = 127 * 65793                    # the largest positive low part (digits 0-2 all +127)
NPERM = 40
NPERM_FLUSH = (255, 256, 511)           # around the 8-bit LDS counters' flush (every 255 permutations)
SUM_BANDS = ('(0,1]', '(1,2]', '(2,4]')                          # |S_p - O| / (members x MF_LO_MAX)
Z_BANDS = ('(0,2^-21]', '(2^-21,2^-18]', '(2^-18,2^-15]')        # |rho_p / rho - 1|


def split_digits(q):
    """q (integers) -> (hi, lo) with q = hi 2^24 + lo and lo = balanced digits 0-2, in [-MF_LO_MAX, LO_TOP]."""
    q = np.asarray(q, dtype=np.int64)
    lo = (q + MF_LO_MAX) % (1 << 24) - MF_LO_MAX
    return (q - lo) >> 24, lo


def image(b):
    """The fixed-point image of an integer-valued f64 matrix: (q int64 with NaN -> 0, present)."""
    b = np.asarray(b, dtype=np.float64)
    present = ~np.isnan(b)
    b0 = np.where(present, b, 0.0)
    q = b0.astype(np.int64)
    assert (q.astype(np.float64) == b0).all(), 'the designed inputs are integers'
    return q, present


class Case:
    def __init__(self, name, score, xy, radius, b, seed, nperms=(NPERM,)):
        self.name, self.score, self.xy, self.radius, self.b, self.seed, self.nperms = name, score, xy, radius, b, seed, nperms
        self._a = None

    @property
    def a(self):
        """Dense 0/1 membership, the oracle's rule (distance < radius x x-range, diagonal kept)."""
        if self._a is None:
            self._a = orc.neighborhoods_euclidean(self.xy, self.radius)
        return self._a

    @property
    def nr(self):
        return orc.layout_radius(self.xy[:, 0], self.radius)


# ---------------------------------------------------------------------------------------------------------------------
# 'sum' families
# ---------------------------------------------------------------------------------------------------------------------
def _lo_draw(rng, shape):
    """Low parts: ~35 % at each end of their range, ~10 % of 0 / +-1, the rest uniform."""
    u = rng.uniform(size=shape)
    lo = rng.integers(-MF_LO_MAX, LO_TOP + 1, size=shape)
    lo = np.where(u < 0.80, rng.integers(-1, 2, size=shape), lo)
    lo = np.where(u < 0.70, LO_TOP, lo)
    lo = np.where(u < 0.35, -MF_LO_MAX, lo)
    return lo.astype(np.int64)


def _ensure_odd(q, rng):
    """Every column needs one odd value (the unit of its image is then 1): add 1 to one row where there is none."""
    for j in range(q.shape[1]):
        if not (q[:, j] & 1).any():
            q[rng.integers(1, q.shape[0]), j] += 1
    return q


def _sum_matrix(rng, n, m, offset, h_lo, h_hi):
    q = offset + (rng.integers(h_lo, h_hi + 1, size=(n, m)).astype(np.int64) << 24) + _lo_draw(rng, (n, m))
    return q


@functools.lru_cache(maxsize=None)
def s_offset():
    """n = 600, radius 0.09 (1-26 members); 2^40 + h 2^24 + lo, h in 0..8.  Column 5 is one value everywhere (every compare a
    tie), column 7 one value but for a spike on three adjacent nodes (the rows that hold all three see every permuted sum
    certainly smaller: their 8-bit field counts to 255 between two flushes), ~3 % of the rows are NaN (never move; NaN -> 0
    shifts a sum by 2^40).  Twelve columns: a launch covers at most 128 permutations and its list of undecided compares holds
    at least 2^20 entries, so with n x m x 128 <= 2^20 the filtered forms cannot overflow into the classic form, whatever
    share of the compares they leave open (the same holds for the 400 x 18 z-score families)."""
    rng = np.random.default_rng(20240601)
    n, m = 600, 12
    xy = rng.uniform(size=(n, 2))
    q = _sum_matrix(rng, n, m, 1 << 40, 0, 8)
    q[:, 5] = (1 << 40) + 12345
    q[:, 7] = (1 << 40) + 1
    b = _ensure_odd(q, rng).astype(np.float64)
    nan_rows = rng.choice(n, n * 3 // 100, replace=False)
    spike = int(np.setdiff1d(np.arange(n), nan_rows)[n // 2])
    near = np.argsort(np.hypot(*(xy - xy[spike]).T) + 10.0 * np.isin(np.arange(n), nan_rows))[:3]
    b[near, 7] += 2.0 ** np.array([36, 35, 34])                         # (the node itself and its two nearest neighbors)
    b[nan_rows] = np.nan
    return Case('S-offset', 'sum', xy, 0.09, b, 17, (NPERM,) + NPERM_FLUSH)


@functools.lru_cache(maxsize=None)
def s_dense():
    """n = 900, radius 0.2, two densities (600 nodes in the left half, 300 in the right): the window of a task comes from its
    GROUP's largest neighborhood, b' from each row's own member count.  h in 0..24."""
    rng = np.random.default_rng(20240602)
    n, m = 900, 12
    xy = rng.uniform(size=(n, 2))
    xy[:600, 0] *= 0.5
    xy[600:, 0] = 0.5 + 0.5 * xy[600:, 0]
    xy = xy[rng.permutation(n)]
    q = _ensure_odd(_sum_matrix(rng, n, m, 1 << 40, 0, 24), rng)
    return Case('S-dense', 'sum', xy, 0.2, q.astype(np.float64), 23)


@functools.lru_cache(maxsize=None)
def s_zero():
    """n = 600, radius 0.09; h 2^24 + lo with h in -5..5 (no offset): observed sums of both signs around zero, where
    (O - b') >> 28 is the floor of a NEGATIVE number.  Row 0 of every column is 2^40 (the column still needs six slices).
    Column 3 has no low digits and h in {-1, 0, 0, 0, 1}: many observed sums are exactly 0.  The last column is negated
    throughout (its largest magnitude is negative)."""
    rng = np.random.default_rng(20240603)
    n, m = 600, 16
    xy = rng.uniform(size=(n, 2))
    q = _sum_matrix(rng, n, m, 0, -5, 5)
    q[:, 3] = rng.choice(np.array([-1, 0, 0, 0, 1], dtype=np.int64), size=n) << 24
    q[0, :] = 1 << 40
    q = _ensure_odd(q, rng)
    q[:, m - 1] = -q[:, m - 1]
    return Case('S-zero', 'sum', xy, 0.09, q.astype(np.float64), 29)


@functools.lru_cache(maxsize=None)
def s_top(hub):
    """A tight cluster of `hub` nodes (each other's neighbors, and nobody else's): one neighborhood size of exactly `hub`
    members, 2047 (the last that k_permtest_mfma_g takes) or 2048; ~250 more nodes around it.  Values at the top of the 47-bit
    range, +-(2^46 - 1 - k 2^24) + lo with k in 1..768: column 0 all positive (observed sums reach 2^57: the headroom of the
    32-bit thresholds), column 1 all negative, columns 2 and 3 of mixed sign."""
    rng = np.random.default_rng(20240604)
    n_out, m = 253, 4
    radius = 0.05
    out = np.empty((0, 2))
    while out.shape[0] < n_out:                                          # uniform, but clear of the cluster
        p = rng.uniform(size=(4 * n_out, 2))
        out = np.concatenate([out, p[np.hypot(p[:, 0] - 0.5, p[:, 1] - 0.5) > 2.5 * radius]])[:n_out]
    out[0], out[1] = (0.0, 0.0), (1.0, 1.0)                              # x-range exactly 1: the radius is `radius`
    ang, rad = rng.uniform(0, 2 * np.pi, hub), 0.004 * np.sqrt(rng.uniform(size=hub))
    xy = np.concatenate([out, 0.5 + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)])
    xy = xy[rng.permutation(xy.shape[0])]
    n = xy.shape[0]
    mag = (1 << 46) - 1 - (rng.integers(1, 769, size=(n, m)).astype(np.int64) << 24)
    sign = np.ones((n, m), dtype=np.int64)
    sign[:, 1] = -1
    sign[:, 2] = np.where(rng.uniform(size=n) < 0.5, 1, -1)
    sign[:, 3] = np.where(rng.uniform(size=n) < 0.1, -1, 1)
    q = _ensure_odd(sign * mag + _lo_draw(rng, (n, m)), rng)
    return Case('S-top-%d' % hub, 'sum', xy, radius, q.astype(np.float64), 31)


# ---------------------------------------------------------------------------------------------------------------------
# z-score families
# ---------------------------------------------------------------------------------------------------------------------
Z_E0_COL, Z_SYM_COL = 16, 17


def _z_near_matrix(rng, n):
    """18 columns of 2^21 L (2^22 + e), L in {3, 5}: |e| <= 6, 40, 300, 2500, two columns each, once as they are and once
    negated throughout (observed scores below zero); column 16 with e = 0 (exact score ties); column 17 with a sign per row
    (sums of values near zero).  One row per column carries + 1: the column's unit."""
    cols = []

    def column(e_max, sign):
        lvl = rng.choice(np.array([3, 5], dtype=np.int64), size=n)
        e = rng.integers(-e_max, e_max + 1, size=n) if e_max else np.zeros(n, dtype=np.int64)
        col = sign * ((lvl * ((1 << 22) + e)) << 21)
        col[rng.integers(0, n)] += 1
        cols.append(col)

    for e_max in (6, 40, 300, 2500):
        for _ in range(2):
            column(e_max, 1)
            column(e_max, -1)
    column(0, 1)
    column(40, np.where(rng.uniform(size=n) < 0.5, 1, -1).astype(np.int64))
    return np.stack(cols, axis=1)


@functools.lru_cache(maxsize=None)
def z_near():
    rng = np.random.default_rng(20240605)
    n = 400
    xy = rng.uniform(size=(n, 2))
    return Case('Z-near', 'z-score', xy, 0.055, _z_near_matrix(rng, n).astype(np.float64), 37, (NPERM,) + NPERM_FLUSH)


@functools.lru_cache(maxsize=None)
def z_var():
    """b = 2^45 + s g, g a fixed pattern of small integers, s so that sd / mean = 2^-11 .. 2^-7, two columns each (the second
    with the pattern reversed): "variance clearly positive" (V > e_v, with its 2^-18 term) turns at sd / mean ~ 2^-9."""
    rng = np.random.default_rng(20240606)
    n = 400
    xy = rng.uniform(size=(n, 2))
    g = rng.integers(-8, 9, size=n).astype(np.int64)
    sd = float(np.std(g))
    cols = []
    for k in (11, 10, 9, 8, 7):
        s = int(round(2.0 ** (45 - k) / sd))
        for pattern in (g, g[::-1]):
            col = (1 << 45) + s * pattern
            col[rng.integers(0, n)] += 1 - (s & 1)                      # (s g is even or odd throughout: make one value odd)
            cols.append(col)
    q = _ensure_odd(np.stack(cols, axis=1), rng)
    return Case('Z-var', 'z-score', xy, 0.055, q.astype(np.float64), 41)


@functools.lru_cache(maxsize=None)
def z_count():
    """Z-near's values with 30 % missing on a radius-0.04 layout: 1-6 members, the number of PRESENT values crosses 3."""
    rng = np.random.default_rng(20240607)
    n = 400
    xy = rng.uniform(size=(n, 2))
    b = _z_near_matrix(rng, n).astype(np.float64)
    b[rng.uniform(size=b.shape) < 0.3] = np.nan
    for j in range(b.shape[1]):                                          # keep the odd value of every column
        col = b[:, j]
        if not (np.nan_to_num(col).astype(np.int64) & 1).any():
            r = int(np.flatnonzero(~np.isnan(col))[0])
            col[r] += 1.0
    return Case('Z-count', 'z-score', xy, 0.04, b, 43)


@functools.lru_cache(maxsize=None)
def z_exact():
    """Z-near's e = 0 column and its symmetric column on grids that keep the SQUARES exact (span <= 23 bits: L alone, and
    +-L (2^22 + e) with e a multiple of 16) -- here the oracle's f64 sums are exact too, and its counters are a reference."""
    rng = np.random.default_rng(20240608)
    n = 400
    xy = rng.uniform(size=(n, 2))
    lvl = rng.choice(np.array([3, 5], dtype=np.int64), size=(n, 2))
    e = 16 * rng.integers(-3, 4, size=n)
    sym = np.where(rng.uniform(size=n) < 0.5, 1, -1) * lvl[:, 1] * ((1 << 22) + e)
    q = np.stack([lvl[:, 0] << 43, sym << 21], axis=1)
    return Case('Z-exact', 'z-score', xy, 0.055, q.astype(np.float64), 47)


@functools.lru_cache(maxsize=None)
def z_low():
    """b = h 2^24 + lo with h in 64..127 and lo mostly at the two ends of the low part (the 'sum' families' draw): the high sums
    are ~100 x the bound d on the low parts, so d (2 |u| + d) and rho gamma c d -- not the single-precision terms, which
    dominate at the top of the range -- are what e_t, e_v and m_s consist of here, and scores within a percent of each other are
    common.  Four columns as they are, two negated throughout, two with a sign per row (|u| around d: s_pos / s_neg)."""
    rng = np.random.default_rng(20240609)
    n, m = 400, 8
    xy = rng.uniform(size=(n, 2))
    q = _sum_matrix(rng, n, m, 0, 64, 127)
    q[:, 4:6] *= -1
    q[:, 6:8] *= np.where(rng.uniform(size=(n, 2)) < 0.5, 1, -1)
    return Case('Z-low', 'z-score', xy, 0.055, _ensure_odd(q, rng).astype(np.float64), 53)


SUM_CASES = {'S-offset': s_offset, 'S-dense': s_dense, 'S-zero': s_zero,
             'S-top-2047': lambda: s_top(2047), 'S-top-2048': lambda: s_top(2048)}
Z_CASES = {'Z-near': z_near, 'Z-var': z_var, 'Z-count': z_count, 'Z-low': z_low, 'Z-exact': z_exact}
CASES = dict(SUM_CASES, **Z_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------------
def _members(a):
    return sp.csr_matrix(np.asarray(a, dtype=np.int64))


def exact_sums(a, b):
    """Observed 'sum' scores as exact integers (int64; the designed sums stay below 2^58)."""
    q, _ = image(b)
    acsr = _members(a)
    assert int(acsr.sum(axis=1).max()) * int(np.abs(q).max()) < 1 << 62
    return acsr @ q


def _permuted_sums(acsr, q, tables):
    for t in np.asarray(tables, dtype=np.int64):
        yield acsr @ q[t]                                                # permuted matrix p = B[table[p]]


def exact_counts(a, b, tables, score='sum'):
    """(#<=, #>=) of the permuted 'sum' scores against the observed ones, int64 [n, m]: gather-sums and compares in integers.
    tables: [P, n] composed row indices, permuted matrix p = B[tables[p]] (Permutations.read, or the oracle's
    permutation_index_table)."""
    if score != 'sum':
        raise ValueError("the exact integer reference covers 'sum' scores (z-scores: the seven-slice form is the reference)")
    q, _ = image(b)
    acsr = _members(a)
    obs = exact_sums(a, b)
    neg, pos = np.zeros(obs.shape, dtype=np.int64), np.zeros(obs.shape, dtype=np.int64)
    for s in _permuted_sums(acsr, q, tables):
        neg += s <= obs
        pos += s >= obs
    return neg, pos


# ---------------------------------------------------------------------------------------------------------------------
# band census: how many of a case's live compares sit near the margins (a property of the INPUTS alone)
# ---------------------------------------------------------------------------------------------------------------------
def _census_sum(a, b, tables):
    q, _ = image(b)
    acsr = _members(a)
    obs = acsr @ q
    unit = np.asarray(acsr.sum(axis=1)).reshape(-1, 1) * MF_LO_MAX      # members x MF_LO_MAX: the bound on a sum of low parts
    hits, live = np.zeros(3, dtype=np.int64), 0
    for s in _permuted_sums(acsr, q, tables):
        d = np.abs(s - obs)
        hits += [np.count_nonzero((d > 0) & (d <= unit)), np.count_nonzero((d > unit) & (d <= 2 * unit)),
                 np.count_nonzero((d > 2 * unit) & (d <= 4 * unit))]
        live += d.size
    return hits / live


def _z_parts(acsr, q, present):
    """Per neighborhood: S1 (int64), count (int64), and N = S1^2, D = count x S2 as Python integers (rho = N / D)."""
    hi, lo = split_digits(q)                                             # squares pass 2^63: three int64 parts, joined as Python ints
    s1, c = acsr @ q, acsr @ present.astype(np.int64)
    s2 = ((acsr @ (hi * hi)).astype(object) << 48) + ((acsr @ (2 * hi * lo)).astype(object) << 24) + (acsr @ (lo * lo)).astype(object)
    s1o = s1.astype(object)
    return s1, c, s1o * s1o, c.astype(object) * s2


def _census_z(a, b, tables):
    q, present = image(b)
    acsr = _members(a)
    s1, c, num, den = _z_parts(acsr, q, present)
    ok = (c >= 3) & np.asarray(den > num, dtype=bool)                    # a score exists: >= 3 values, variance > 0
    hits, live = np.zeros(3, dtype=np.int64), 0
    for t in np.asarray(tables, dtype=np.int64):
        s1p, cp, nump, denp = _z_parts(acsr, q[t], present[t])
        both = ok & (cp >= 3) & np.asarray(denp > nump, dtype=bool)
        live += np.count_nonzero(both)
        near = both & (np.sign(s1p) == np.sign(s1)) & (s1 != 0)
        # |rho_p / rho - 1| = |N_p D - D_p N| / (D_p N)
        r, base = np.abs(nump * den - denp * num)[near], (denp * num)[near]
        in21, in18, in15 = (np.asarray((r << k) <= base, dtype=bool) for k in (21, 18, 15))
        hits += [np.count_nonzero(in21 & np.asarray(r > 0, dtype=bool)), np.count_nonzero(in18 & ~in21), np.count_nonzero(in15 & ~in18)]
    return hits / max(live, 1)


def band_census(case, tables=None):
    """Share of the case's live compares in each of the three bands next to the margins, in exact integer arithmetic:
    'sum'  |S_p - O| / (members x MF_LO_MAX) in (0,1], (1,2], (2,4];
    z      |rho_p / rho - 1| in (0, 2^-21], (2^-21, 2^-18], (2^-18, 2^-15], rho = S1^2 / (count x S2), over the compares where
           both scores exist (same sign of S1; exact squares -- the image rounds them by 2^-46 relative).
    tables default to the oracle's stream for the case's seed and NPERM permutations."""
    if tables is None:
        tables = orc.permutation_index_table(case.b, NPERM, case.seed)
    return (_census_sum if case.score == 'sum' else _census_z)(case.a, case.b, tables)
