"""The reference of the analytic test (how = 'analytic'; include/safe_hip.h: safe_moments_test, safe_attr_column_moments) and
the designed inputs of tests/test_gpu_moments.py.  No device, no safepy_amd import.

Definition.  Population of a column: the rows with at least one value (row flag 1); a NaN cell inside them counts as 0.  With
n_v such rows, mu = column sum / n_v, Q = sum over them of (b - mu)^2, k = members of a neighborhood that are in the
population and x = the neighborhood's sum,

    var = k (n_v - k) / (n_v (n_v - 1)) * Q        z = (x - k mu) / sqrt(var)        P[Z >= z] = erfc(z / sqrt 2) / 2

and a cell with n_v < 2, k = 0, k = n_v or Q = 0 is degenerate: p_pos = p_neg = 1, z = 0.  mu, Q, var and z^2 are exact
rationals (fractions.Fraction); the root and erfc are mpmath at 50 digits.
"""
import itertools
import math
from fractions import Fraction

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50

U = 2.0 ** -53
Z_EDGE = 37.5                   # beyond it the small side may be anything in [0, SMALL_MAX] and the large side is 1
SMALL_MAX = 2.3e-308
SIGNS = ('highest', 'lowest', 'both')


def to_mp(v):
    if isinstance(v, Fraction):
        return MP.mpf(v.numerator) / MP.mpf(v.denominator)
    return MP.mpf(float(v))


def row_flags(b):
    b = np.asarray(b)
    if not np.issubdtype(b.dtype, np.floating):
        return np.ones(b.shape[0], dtype=bool)
    return (~np.isnan(b)).any(axis=1)


def exact_column(values):
    """(mu, Q) of one column's population values (NaN already 0) as Fractions."""
    vals = [Fraction(float(v)) for v in values]
    if not vals:
        return Fraction(0), Fraction(0)
    mu = sum(vals, Fraction(0)) / len(vals)
    return mu, sum(((v - mu) ** 2 for v in vals), Fraction(0))


def exact_moments(b):
    """(flags, n_v, [mu_j], [Q_j]) of a dense matrix."""
    b = np.asarray(b)
    flags = row_flags(b)
    pop = np.nan_to_num(b[flags].astype(np.float64))
    cols = [exact_column(pop[:, j]) for j in range(b.shape[1])]
    return flags, int(flags.sum()), [c[0] for c in cols], [c[1] for c in cols]


def exact_css_about(values, centre):
    """sum (v - centre)^2 as a Fraction, centre a float (the device's own mean)."""
    c = Fraction(float(centre))
    return sum(((Fraction(float(v)) - c) ** 2 for v in values), Fraction(0))


def exact_var(k, n_v, q):
    if n_v < 2:
        return Fraction(0)
    return Fraction(k * (n_v - k), n_v * (n_v - 1)) * q


def exact_z(x, k, n_v, mu, q):
    """(z, sd, k mu) as mpmath numbers; (None, None, None) for a degenerate cell.  x, mu, q: Fractions or floats (exact)."""
    x, mu, q = (v if isinstance(v, Fraction) else Fraction(float(v)) for v in (x, mu, q))
    var = exact_var(int(k), int(n_v), q)
    if var <= 0:
        return None, None, None
    d = x - int(k) * mu
    z = MP.sqrt(to_mp(d * d / var))
    return (-z if d < 0 else z), MP.sqrt(to_mp(var)), to_mp(int(k) * mu)


def small_side(z):
    """P[Z >= |z|] for a standard normal Z, as an mpmath number."""
    return MP.erfc(abs(MP.mpf(z)) / MP.sqrt(2)) / 2


def upper_tail(z):
    return MP.erfc(MP.mpf(z) / MP.sqrt(2)) / 2


def k_ref(z_list, tail=None):
    """The measured constant of the p-value bound: the largest relative error of scipy.special.ndtr(-z) -- the function behind
    scipy.stats.norm.sf -- against mpmath over z_list (|z| <= Z_EDGE), in units of (1 + z^2) 2^-53.  tail: another P[Z >= z]
    to measure the same way."""
    from scipy.special import ndtr
    tail = tail or (lambda z: ndtr(-z))
    worst = 0.0
    for z in z_list:
        z = float(z)
        if not abs(z) <= Z_EDGE:
            continue
        want = upper_tail(z)
        err = abs(MP.mpf(float(tail(z))) - want) / want
        worst = max(worst, float(err / ((1 + MP.mpf(z) ** 2) * U)))
    return worst


def p_cut(threshold):
    """nes_p_cut of the library (common.h) restated: the smallest double whose -log10 (libm) does not exceed -log10(threshold)."""
    thr = -math.log10(threshold)
    hit = lambda p: -math.log10(p) > thr                        # noqa: E731
    p = threshold
    for _ in range(4096):
        if not hit(p):
            break
        p = math.nextafter(p, 1.0)
    for _ in range(4096):
        if hit(math.nextafter(p, 0.0)):
            break
        p = math.nextafter(p, 0.0)
    return p


def decisions(p_pos, p_neg, nes, sign, threshold):
    """nes_binary from the device's own p-values (one side: p < p_cut) or its own nes ('both': |nes| > -log10 threshold)."""
    if sign == 'highest':
        return (p_pos < p_cut(threshold)).astype(np.float64)
    if sign == 'lowest':
        return (p_neg < p_cut(threshold)).astype(np.float64)
    with np.errstate(invalid='ignore'):
        return ((np.abs(nes) > -math.log10(threshold)) & ~np.isnan(nes)).astype(np.float64)


def nes_of(p_pos, p_neg, sign):
    with np.errstate(divide='ignore'):
        ep, en = -np.log10(p_pos), -np.log10(p_neg)
    return ep if sign == 'highest' else en if sign == 'lowest' else ep - en


# ---- brute force ------------------------------------------------------------------------------------------------------------

def enumerated_moments(column, flags, members):
    """Mean and variance (exact) of the neighborhood sum over ALL permutations of the population rows' values (the rows without
    a value stay where they are and add 0; NaN cells inside the population count as 0)."""
    idx = [i for i, f in enumerate(flags) if f]
    vals = [Fraction(0) if v != v else Fraction(float(v)) for v in (column[i] for i in idx)]
    inside = [pos for pos, i in enumerate(idx) if members[i]]
    sums = [sum((perm[pos] for pos in inside), Fraction(0)) for perm in itertools.permutations(vals)]
    mean = sum(sums, Fraction(0)) / len(sums)
    return mean, sum(((s - mean) ** 2 for s in sums), Fraction(0)) / len(sums)


# ---- the designed inputs of the GPU test ------------------------------------------------------------------------------------

class Case:
    """a: membership [n, n] (0/1), b: attributes [n, m] f64 with NaN; the facts the checks need, from the reference alone."""

    def __init__(self, name, a, b):
        self.name, self.a, self.b = name, np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        self.flags = row_flags(self.b)
        self.n_v = int(self.flags.sum())
        self.k = (self.a @ self.flags.astype(np.float64)).astype(np.int64)
        self.x = self.a @ np.nan_to_num(self.b)                 # (integers far below 2^53 in every designed case: exact)
        self._exact = None

    def _moments(self):
        if self._exact is None:                                 # (Fractions: only the cases that ask pay for them)
            self._exact = exact_moments(self.b)[2:]
        return self._exact

    @property
    def mu(self):
        return self._moments()[0]

    @property
    def q(self):
        return self._moments()[1]

    def cells(self):
        """{(k, column, x): exact z or None} over the distinct cells."""
        out = {}
        n, m = self.b.shape
        for j in range(m):
            for key in set(zip(self.k.tolist(), self.x[:, j].tolist())):
                out[(key[0], j, key[1])] = exact_z(Fraction(key[1]), key[0], self.n_v, self.mu[j], self.q[j])[0]
        return out


N_V = 2048
N_MISSING = 32
SIZES = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 96, 128, 192, 256, 512, 1024, 2047)
HEADS = (0, 1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)
ONES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2040)


def designed_columns():
    """Integer columns over N_V population rows, every one non-increasing in the row index (so 'the h first rows' are the h
    largest values), |b| <= 1024, n_v a power of two: every mean is exact in f64."""
    r = np.arange(N_V)
    cols = [(r < k).astype(np.float64) for k in ONES]
    cols += [np.maximum(0, 7 - r // s).astype(np.float64) for s in (1, 4, 32, 128)]
    cols.append(np.where(r < 100, 3.0, np.where(r >= 1900, -2.0, 0.0)))
    cols.append(np.where(r < 5, 1024.0, 0.0))
    cols.append(np.where(r >= 2040, -1024.0, 0.0))
    cols.append(np.full(N_V, 3.0))                              # constant columns: degenerate
    cols.append(np.zeros(N_V))
    holes = (r < 64).astype(np.float64)
    holes[1000:1100] = np.nan                                   # NaN cells inside rows that have a value: they count as 0
    cols.append(holes)
    return np.stack(cols, axis=1)


def designed_neighborhoods():
    """(k, h): the h first population rows (the largest values of every column) plus the k - h last ones."""
    pairs = []
    for k in SIZES:
        for h in sorted(set(v for v in HEADS + (k // 2, k - 1, k) if 0 <= v <= k)):
            pairs.append((k, h))
    return pairs


def designed_case():
    n = N_V + N_MISSING
    b = np.full((n, designed_columns().shape[1]), np.nan)
    b[:N_V] = designed_columns()
    b[5, -2] = np.nan                                           # (a NaN cell in a constant-zero column changes nothing)
    pairs = designed_neighborhoods()
    a = np.zeros((n, n))
    for i in range(n):
        k, h = pairs[i % len(pairs)]
        a[i, :h] = 1
        a[i, N_V - (k - h):N_V] = 1
        if i % 3 == 0:
            a[i, N_V + i % N_MISSING] = 1                       # a member without a value: adds 0, is not counted in k
    a[n - 1] = 0
    a[n - 1, :N_V] = 1                                          # k = n_v
    a[n - 2] = 0
    a[n - 2, N_V:] = 1                                          # k = 0: only members without a value
    return Case('designed', a, b)


def lonely_case():
    """n_v = 1: every cell is degenerate."""
    b = np.full((3, 2), np.nan)
    b[1] = (2.0, 0.0)
    return Case('n_v = 1', np.array([[1, 1, 0], [0, 1, 0], [1, 1, 1.0]]), b)


_DESIGNED = {}


def designed():
    """The designed cases, built once."""
    if not _DESIGNED:
        _DESIGNED['cases'] = (designed_case(), lonely_case())
    return _DESIGNED['cases']


def designed_z():
    """Every exact z of the designed cells correctly rounded to f64 (the GPU test's own z list), and the number of degenerate
    cells by kind."""
    if 'z' not in _DESIGNED:
        zs, kinds = [], {'n_v < 2': 0, 'k = 0': 0, 'k = n_v': 0, 'constant column': 0}
        for case in designed():
            for (k, j, _), z in case.cells().items():
                if z is not None:
                    zs.append(float(z))
                elif case.n_v < 2:
                    kinds['n_v < 2'] += 1
                elif k == 0:
                    kinds['k = 0'] += 1
                elif k == case.n_v:
                    kinds['k = n_v'] += 1
                else:
                    assert case.q[j] == 0
                    kinds['constant column'] += 1
        _DESIGNED['z'] = (np.array(sorted(set(zs))), kinds)
    return _DESIGNED['z']


def designed_k_ref():
    if 'k_ref' not in _DESIGNED:
        _DESIGNED['k_ref'] = k_ref(designed_z()[0])
    return _DESIGNED['k_ref']


def periodic_case(n, m, seed, integers=False, missing=True):
    """A shape-sweep input: real (or small non-negative integer) values, but only 5 distinct neighborhoods and 7 distinct
    columns whatever n and m are, so the exact checks visit at most 35 distinct cells while every cell of the output is compared
    with its representative's bits."""
    rng = np.random.default_rng(seed)
    pats = rng.integers(0, 4, size=(n, 7)).astype(np.float64) if integers else np.round(rng.normal(size=(n, 7)) * 3, 3)
    if missing and n >= 4:
        pats[rng.choice(n, max(1, n // 8), replace=False)] = np.nan            # rows without a value
        holes = rng.uniform(size=pats.shape) < 0.05
        pats[holes & ~np.isnan(pats).all(axis=1)[:, None]] = np.nan            # NaN cells (a row may lose all its values too)
    if n >= 3:
        pats[:, 6] = pats[0, 6] if pats[0, 6] == pats[0, 6] else 1.0           # a constant column ...
        if missing and n >= 4:
            pats[np.isnan(pats[:, :6]).all(axis=1), 6] = np.nan                # ... over the rows that have a value
    b = pats[:, np.arange(m) % 7]
    rows = (rng.uniform(size=(5, n)) < np.array([0.1, 0.3, 0.5, 0.9, 1.0])[:, None]).astype(np.float64)
    rows[:, 0] = 1
    return Case('periodic %d x %d' % (n, m), rows[np.arange(n) % 5], b)
