"""The reference of the max-statistic adjustment (include/safe_hip.h: safe_permtest_extremes, safe_counts_from_extremes) and the
inputs its tests share.  NumPy only: no device, no safepy_amd import.

Definition.  S_p[i, j]: the permuted 'sum' score, members added in ascending node order, one accumulator per cell, NaN -> 0,
weight 1.0 on a flat membership (weights_ref.score).  loc_i, scale_i: k_i and f_i = k_i (n_v - k_i) / (n_v (n_v - 1)) on a flat
membership, W1_i and g_i of weights_ref.row_sums on a weighted one.  mu_j, Q_j: the column moments, given (on the device those
of safe_attr_column_moments).  var = scale_i Q_j;  z = (S - loc_i mu_j) / sqrt(var) where var > 0, else the cell is degenerate
and z = 0.  tmax[p, j] / tmin[p, j]: the extremes of z_p over the non-degenerate rows, -inf / +inf without one.
"""
import numpy as np

import weights_ref as wr

COLUMN, MATRIX = 0, 1       # SAFE_FAMILY_*


def column_moments(b, flags):
    """(mu, Q) of every column over the flagged rows, NaN as 0, Q = 0 for a constant column: plain NumPy, for the checks that
    need no device (the device's own bits come from Attributes.column_moments)."""
    v = np.nan_to_num(np.asarray(b, dtype=np.float64))[np.asarray(flags, dtype=bool)]
    if len(v) == 0:
        return np.zeros(v.shape[1]), np.zeros(v.shape[1])
    mu = v.sum(axis=0) / len(v)
    q = ((v - mu) ** 2).sum(axis=0)
    q[v.min(axis=0) == v.max(axis=0)] = 0.0
    return mu, q


def row_factors(indptr, indices, flags, n_v, w=None):
    """(loc, scale) f64 [n]: k_i, f_i on a flat membership (w None), W1_i, g_i with weights."""
    flags = np.asarray(flags, dtype=bool)
    if w is not None:
        w1, _, _, g = wr.row_sums(indptr, indices, np.asarray(w, dtype=np.float64), flags, n_v)
        return w1, g
    n = len(indptr) - 1
    k = np.array([np.count_nonzero(flags[indices[indptr[i]:indptr[i + 1]]]) for i in range(n)], dtype=np.float64)
    nv = float(n_v)
    f = np.zeros(n)
    ok = (k > 0) & (k < nv) if nv >= 2 else np.zeros(n, dtype=bool)
    f[ok] = (k[ok] * (nv - k[ok])) / (nv * (nv - 1.0))
    return k, f


def standardise(s, loc, scale, mu, q):
    """(z, live): z = (s - loc mu) / sqrt(scale q) where scale q > 0, 0 elsewhere."""
    var = scale[:, None] * q[None, :]
    live = var > 0.0
    z = np.zeros(s.shape)
    centre = loc[:, None] * mu[None, :]
    z[live] = (s[live] - centre[live]) / np.sqrt(var[live])
    return z, live


def extremes(indptr, indices, w, b, tables, loc, scale, mu, q):
    """(z_obs [n, m], live [n, m], tmax [P, m], tmin [P, m], z_all [P, n, m]); w None = a flat membership."""
    ww = np.ones(len(indices)) if w is None else np.asarray(w, dtype=np.float64)
    z_obs, live = standardise(wr.score(indptr, indices, ww, b), loc, scale, mu, q)
    tables = np.asarray(tables)
    m = np.asarray(b).shape[1]
    tmax, tmin = np.full((len(tables), m), -np.inf), np.full((len(tables), m), np.inf)
    z_all = np.zeros((len(tables),) + z_obs.shape)
    for p, t in enumerate(tables):
        z, _ = standardise(wr.score(indptr, indices, ww, b, source_rows=t), loc, scale, mu, q)
        z_all[p] = z
        tmax[p] = np.where(live, z, -np.inf).max(axis=0, initial=-np.inf)
        tmin[p] = np.where(live, z, np.inf).min(axis=0, initial=np.inf)
    return z_obs, live, tmax, tmin, z_all


def counts(z_obs, live, tmax, tmin, scope):
    """(counts_neg, counts_pos [n, m], min_counts_neg, min_counts_pos [m]) as f64."""
    P = len(tmax)
    if scope == MATRIX:
        hi = np.broadcast_to(tmax.max(axis=1)[:, None], tmax.shape)
        lo = np.broadcast_to(tmin.min(axis=1)[:, None], tmin.shape)
    else:
        hi, lo = tmax, tmin
    pos = (hi[:, None, :] >= z_obs[None, :, :]).sum(axis=0).astype(np.float64)
    neg = (lo[:, None, :] <= z_obs[None, :, :]).sum(axis=0).astype(np.float64)
    pos[~live] = P
    neg[~live] = P
    least_neg = np.where(live, neg, P).min(axis=0, initial=P).astype(np.float64)
    least_pos = np.where(live, pos, P).min(axis=0, initial=P).astype(np.float64)
    return neg, pos, least_neg, least_pos


def raw_counts(z_obs, z_all):
    """#{p : z_p >= z_obs}, #{p : z_p <= z_obs} per cell: the unadjusted permutation counts on the same statistic."""
    return (z_all <= z_obs[None]).sum(axis=0).astype(np.float64), (z_all >= z_obs[None]).sum(axis=0).astype(np.float64)


# ---- shared inputs ------------------------------------------------------------------------------------------------------------

def lattice(side, reach):
    """(xy [side^2, 2], membership [n, n] bool): the nodes of a side x side lattice, members within Euclidean distance `reach`."""
    g = np.arange(side)
    xy = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2).astype(np.float64)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(axis=-1)
    return xy, d2 <= reach * reach + 1e-9


def planted_lattice(side=18, reach=2.0, m=400, seed=5, centre=40, disc=3.0, lift=1.5):
    """The null example of the issue: standard-normal columns, +lift planted on the disc of radius `disc` around node `centre`
    of column 0.  (xy, a, b, planted nodes)."""
    rng = np.random.default_rng(seed)
    xy, a = lattice(side, reach)
    b = rng.normal(size=(side * side, m))
    planted = np.flatnonzero(((xy - xy[centre]) ** 2).sum(axis=1) <= disc * disc + 1e-9)
    b[planted, 0] += lift
    return xy, a, b, planted


def random_tables(n, flags, count, rng):
    """[count, n] row maps that shuffle the flagged rows among themselves and leave the others in place."""
    movable = np.flatnonzero(np.asarray(flags, dtype=bool))
    out = np.tile(np.arange(n), (count, 1))
    for t in out:
        t[movable] = rng.permutation(movable)
    return out


def tied_case(n, m, seed):
    """Integer data on a membership of equal-sized neighborhoods (a ring, 5 members each): every row has the same loc and scale,
    so equal sums are equal z, and small integers make equal sums frequent -- the >= and <= of the counts are exercised on ties.
    (a [n, n] bool, b [n, m] f64)."""
    rng = np.random.default_rng(seed)
    idx = (np.arange(n)[:, None] + np.arange(-2, 3)[None, :]) % n
    a = np.zeros((n, n), dtype=bool)
    a[np.arange(n)[:, None], idx] = True
    return a, rng.integers(0, 2, size=(n, m)).astype(np.float64)
