"""The reference of the distance-weighted neighborhood scores (include/safe_hip.h: safe_nbr_weights_from_xy, safe_score_weighted,
safe_moments_test_weighted, safe_permtest_counts_weighted) and the designed inputs of tests/test_gpu_weights.py.  NumPy,
Fractions and mpmath only: no device, no safepy_amd import.

Definition.  Members of row i = its CSR entries in ascending column order; D[i, k] the node distance, r_i the row's radius,
u = D / r (0 where r = 0), h the bandwidth:

    uniform 1 | triangular max(0, 1 - u) | epanechnikov max(0, 1 - u u) | gaussian exp(-0.5 (t t)), t = u / h

    x_ij = (((0.0 + w_i,k1 v_k1,j) + w_i,k2 v_k2,j) + ...)      v = the value as f64, NaN -> 0; every operation rounded

Over the members of row i that hold a value (row flag 1), ascending: W1 = sum w, W2 = sum w w, c their number.  With n_v, mu_j,
Q_j of moments_ref:  g_i = (n_v W2 - W1 W1) / (n_v (n_v - 1)),  var = g_i Q_j,  z = (x - W1 mu_j) / sqrt(var);  g_i = 0 when
n_v < 2, c = 0, c = n_v with all flagged weights equal, or the value is not positive.  Under a permutation T of the rows that
hold a value, S[i, j] is x with v taken at row T[k].
"""
import itertools
from fractions import Fraction

import numpy as np

import moments_ref as mr

KINDS = ('uniform', 'triangular', 'epanechnikov', 'gaussian')


# ---- membership and distances -----------------------------------------------------------------------------------------------

def csr_of(a):
    """(indptr int64 [n + 1], indices int64 [nnz]) of a dense 0/1 membership, columns ascending."""
    a = np.asarray(a) != 0
    rows, cols = np.nonzero(a)                                  # row-major: ascending columns inside a row
    return np.concatenate([[0], np.cumsum(a.sum(axis=1))]).astype(np.int64), cols.astype(np.int64)


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def euclidean_member_distances(xy, indptr, indices):
    """sqrt(dx dx + dy dy) of every CSR entry, the bits of scipy's pdist (every operation rounded)."""
    xy = np.asarray(xy, dtype=np.float64)
    i = rows_of(indptr)
    dx = xy[i, 0] - xy[indices, 0]
    dy = xy[i, 1] - xy[indices, 1]
    return np.sqrt(dx * dx + dy * dy)


def matrix_member_distances(dist, indptr, indices):
    return np.asarray(dist, dtype=np.float64)[rows_of(indptr), indices]


# ---- weights ----------------------------------------------------------------------------------------------------------------

def scaled(d, r):
    """u = d / r, 0 where r == 0 (0 / 0 is never evaluated)."""
    d, r = np.broadcast_arrays(np.asarray(d, dtype=np.float64), np.asarray(r, dtype=np.float64))
    return np.divide(d, r, out=np.zeros(d.shape), where=r != 0)


def gaussian_argument(d, r, h):
    t = scaled(d, r) / h
    return -0.5 * (t * t)


def weights(kind, d, r, h=0.5):
    """The weight of every entry; 'gaussian' through np.exp (the device's exp is compared with mpmath instead)."""
    u = scaled(d, r)
    if kind == 'uniform':
        return np.ones(u.shape)
    if kind == 'triangular':
        return np.maximum(0.0, 1.0 - u)
    if kind == 'epanechnikov':
        return np.maximum(0.0, 1.0 - u * u)
    if kind == 'gaussian':
        return np.exp(gaussian_argument(d, r, h))
    raise ValueError(kind)


def member_weights(kind, d, indptr, radii, h=0.5):
    r = np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(indptr) - 1,))
    return weights(kind, d, r[rows_of(indptr)], h)


def exp_correctly_rounded(arg):
    """mpmath's exp of every f64 argument, rounded to nearest f64."""
    mp = mr.MP
    return np.array([float(mp.exp(mp.mpf(float(a)))) for a in np.asarray(arg).ravel()]).reshape(np.shape(arg))


def ulps_from(values, want):
    """|values - want| in units of the spacing of `want` (f64)."""
    values, want = np.asarray(values, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(values - want) / np.spacing(np.abs(want))


def exp_error_ulps(arg, values):
    """The error of `values` as exp(arg) against mpmath at 50 digits, in ulps of the correctly rounded result."""
    mp = mr.MP
    worst = 0.0
    for a, v in zip(np.asarray(arg).ravel().tolist(), np.asarray(values).ravel().tolist()):
        want = mp.exp(mp.mpf(a))
        ulp = float(np.spacing(float(want)))
        worst = max(worst, float(abs(mp.mpf(v) - want) / ulp))
    return worst


# ---- the weighted score -----------------------------------------------------------------------------------------------------

def score(indptr, indices, w, b, source_rows=None, descending=False):
    """x [n, m]: one accumulator per cell, members added in ascending (or, to show that the order matters, descending) order,
    every product and sum rounded.  source_rows: T [n], the value of member k is taken at row T[k]."""
    v = np.where(np.isnan(np.asarray(b, dtype=np.float64)), 0.0, np.asarray(b, dtype=np.float64))
    n = len(indptr) - 1
    counts = np.diff(indptr)
    acc = np.zeros((n, v.shape[1]))
    order = np.argsort(-counts, kind='stable')                  # rows by descending count: the active rows are a prefix
    sorted_counts = counts[order]
    for t in range(int(counts.max()) if n else 0):
        rows = order[:np.searchsorted(-sorted_counts, -t, side='left')]        # rows with count > t
        e = indptr[rows] + (counts[rows] - 1 - t if descending else t)
        k = indices[e]
        if source_rows is not None:
            k = np.asarray(source_rows)[k]
        acc[rows] = acc[rows] + w[e][:, None] * v[k]
    return acc


def counts(indptr, indices, w, b, tables):
    """(x, counts_neg, counts_pos) of the randomization test over the rows of `tables` [P, >= n]."""
    x = score(indptr, indices, w, b)
    neg, pos = np.zeros(x.shape), np.zeros(x.shape)
    for t in np.asarray(tables):
        s = score(indptr, indices, w, b, source_rows=t)
        neg += s <= x
        pos += s >= x
    return x, neg, pos


# ---- the analytic test ------------------------------------------------------------------------------------------------------

def row_sums(indptr, indices, w, flags, n_v):
    """(W1, W2, c, g) of every row in f64, the sums sequential over the flagged members in ascending order, as the contract
    writes them."""
    n = len(indptr) - 1
    w1, w2, c, g = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n)
    nv = float(n_v)
    for i in range(n):
        sel = [e for e in range(indptr[i], indptr[i + 1]) if flags[indices[e]]]
        a = b = 0.0
        for e in sel:
            wt = float(w[e])
            a = a + wt
            b = b + wt * wt
        w1[i], w2[i], c[i] = a, b, len(sel)
        if n_v >= 2 and sel and not (len(sel) == n_v and min(w[sel]) == max(w[sel])):
            val = (nv * b - a * a) / (nv * (nv - 1.0))
            g[i] = val if val > 0.0 else 0.0
    return w1, w2, c, g


def exact_row(w_flagged, n_v):
    """(W1, W2, g) as Fractions from the f64 weights of a row's flagged members; g = 0 in the degenerate cases."""
    ws = [Fraction(float(v)) for v in w_flagged]
    w1, w2 = sum(ws, Fraction(0)), sum((v * v for v in ws), Fraction(0))
    if n_v < 2 or not ws or (len(ws) == n_v and min(ws) == max(ws)):
        return w1, w2, Fraction(0)
    g = (n_v * w2 - w1 * w1) / (n_v * (n_v - 1))
    return w1, w2, max(g, Fraction(0))


def exact_mean_var(w_population, values):
    """Mean and variance of sum_r w_r v_T(r) over the uniform permutations T of the population, in closed form: w_population
    holds the weight of every population row (0 for a non-member), values its value; Fractions."""
    ws = [Fraction(v) for v in w_population]
    vals = [Fraction(v) for v in values]
    n_v = len(vals)
    mu = sum(vals, Fraction(0)) / n_v
    q = sum(((v - mu) ** 2 for v in vals), Fraction(0))
    w1, w2 = sum(ws, Fraction(0)), sum((v * v for v in ws), Fraction(0))
    if n_v < 2:
        return w1 * mu, Fraction(0)
    return w1 * mu, (n_v * w2 - w1 * w1) / (n_v * (n_v - 1)) * q


def enumerated_mean_var(w_population, values):
    """The same two numbers from ALL permutations."""
    ws = [Fraction(v) for v in w_population]
    vals = [Fraction(v) for v in values]
    sums = [sum((a * b for a, b in zip(ws, perm)), Fraction(0)) for perm in itertools.permutations(vals)]
    mean = sum(sums, Fraction(0)) / len(sums)
    return mean, sum(((s - mean) ** 2 for s in sums), Fraction(0)) / len(sums)


def exact_z(x, w1, g, mu, q):
    """(z, sd, W1 mu) as mpmath numbers from exact inputs (Fractions or floats); (None, None, None) for a degenerate cell."""
    x, w1, g, mu, q = (v if isinstance(v, Fraction) else Fraction(float(v)) for v in (x, w1, g, mu, q))
    var = g * q
    if var <= 0:
        return None, None, None
    d = x - w1 * mu
    z = mr.MP.sqrt(mr.to_mp(d * d / var))
    return (-z if d < 0 else z), mr.MP.sqrt(mr.to_mp(var)), mr.to_mp(w1 * mu)


# ---- designed inputs --------------------------------------------------------------------------------------------------------

def designed_weights(indptr, indices):
    """(1 + (i + k) mod 8) / 8 on member k of row i: dyadic, so every sum of the designed case is exact in f64."""
    return (1 + (rows_of(indptr) + indices) % 8) / 8.0


_DESIGNED = {}


def designed():
    """moments_ref.designed_case() with designed_weights: (case, indptr, indices, w), built once."""
    if 'case' not in _DESIGNED:
        case = mr.designed_case()
        indptr, indices = csr_of(case.a)
        _DESIGNED['case'] = (case, indptr, indices, designed_weights(indptr, indices))
    return _DESIGNED['case']


def designed_cells():
    """Per row and column of the designed case, from exact arithmetic: x (Fractions as an object array is too slow: the sums are
    dyadic and small, so the f64 score IS exact -- asserted), W1, W2, g as Fractions per row, and exact_z's (z, sd, W1 mu) per
    distinct cell."""
    if 'cells' not in _DESIGNED:
        case, indptr, indices, w = designed()
        x = score(indptr, indices, w, case.b)
        rows = []
        for i in range(len(indptr) - 1):
            sel = [e for e in range(indptr[i], indptr[i + 1]) if case.flags[indices[e]]]
            rows.append(exact_row(w[sel], case.n_v))
        z = {}
        for j in range(case.b.shape[1]):
            for i in range(len(rows)):
                key = (rows[i][0], rows[i][2], j, x[i, j])
                if key not in z:
                    z[key] = exact_z(Fraction(x[i, j]), rows[i][0], rows[i][2], case.mu[j], case.q[j])
        _DESIGNED['cells'] = (x, rows, z)
    return _DESIGNED['cells']


def order_sensitive(n, m, seed, big_row=None):
    """The 'order-sensitive' input: values round(normal * 3, 3), weights 1 - U(0, 1) on a random membership whose rows hold from
    a handful to (big_row or n) members: (a, b, indptr, indices, w)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n, n)) < rng.uniform(0.02, 0.3, size=(n, 1))
    a[np.arange(n), np.arange(n)] = True
    if big_row is not None:
        a[0, :big_row] = True
    b = np.round(rng.normal(size=(n, m)) * 3, 3)
    indptr, indices = csr_of(a)
    w = 1.0 - rng.uniform(size=len(indices))
    return a.astype(np.int64), b, indptr, indices, w


def gaussian_test_arguments(count=4000, seed=7):
    """Arguments in [-8, 0] of the kind the Gaussian weights produce: -0.5 (u / h)^2 for u in [0, 1], h in (0.25, 0.5, 2)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(size=count)
    h = np.array([0.25, 0.5, 2.0])[rng.integers(0, 3, size=count)]
    t = u / h
    return -0.5 * (t * t)


def k_exp_ref(args=None):
    """The worst error of np.exp against mpmath in ulps on the Gaussian test arguments."""
    if 'k_exp' not in _DESIGNED or args is not None:
        a = gaussian_test_arguments() if args is None else np.asarray(args)
        k = exp_error_ulps(a, np.exp(a))
        if args is not None:
            return k
        _DESIGNED['k_exp'] = k
    return _DESIGNED['k_exp']
