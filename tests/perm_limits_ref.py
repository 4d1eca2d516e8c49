"""Host reference and inputs of tests/test_gpu_perm_limits.py: the permutation test at the resource limits of the LDS-resident f64
kernel (k_permtest_lds) and of the scatter kernel (k_permtest_scatter), safepy_amd/csrc/enrich.hip: perm_route.  NumPy / SciPy
only; no dense N x N matrix is ever built (the memberships are CSR, a neighborhood's score is a sparse product).

The limits, restated from the two byte formulas of enrich.hip (tests/test_perm_limits_ref_cpu.py reads the formulas out of the
source and checks that these are the largest sizes they admit):
  ldsf64_bytes(n, stride16) = 4 (8 (n + 1) + stride16 + 4), stride16 = 8 ceil((n + 1) / 8):   N <= 4549 within 160 KiB
  scatter_lds_bytes(n)      = 4 (2 n + 4) + 2 ((n + 1) & ~1):                                  N <= 16 382 within 160 KiB
  max_count < SC_EPOCH = 4096: a neighborhood of at most 4095 members
  two 16-bit counters in one word (both kernels): at most 65 535 permutations

The counters have exactly one right answer for 'sum' scores of values on a dyadic grid (multiples of 1/16, counts_sum asserts it):
every partial sum is exact, whatever the order.  For z-scores the reference's own rounding decides a compare only where the
permuted score lies within 1e-9 (relative to max(1, |observed|)) of the observed one; counts_z tallies those per cell."""
import numpy as np
import scipy.sparse as sp

LDS_BUDGET = 160 * 1024
LDS_F64_MAX_N = 4549
SCATTER_MAX_N = 16382
SCATTER_MAX_MEMBERS = 4095
PACKED_MAX_P = 65535
GRID = 16.0                                                              # values are multiples of 1 / GRID


def lds_f64_bytes(n):
    stride16 = 8 * ((n + 1 + 7) // 8)
    return 4 * (8 * (n + 1) + stride16 + 4)


def scatter_bytes(n):
    return 4 * (2 * n + 4) + 2 * ((n + 1) & ~1)


# ------------------------------------------------------------------------------------------------- the reference ----

def membership_csr(indptr, indices, n):
    """What Neighborhoods.csr() returns, as a scipy.sparse.csr_matrix of ones."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    assert indptr.shape == (n + 1,) and indptr[0] == 0 and indptr[-1] == indices.shape[0]
    return sp.csr_matrix((np.ones(indices.shape[0]), indices, indptr), shape=(n, n))


def csr_of_dense(a):
    """(indptr, indices) of a dense 0/1 matrix, columns increasing within a row."""
    a = np.asarray(a)
    rows, cols = np.nonzero(a)
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=a.shape[0]))]).astype(np.int64), cols.astype(np.int64)


def _zeroed(b):
    b = np.asarray(b, dtype=np.float64)
    return np.where(np.isnan(b), 0.0, b)


def _assert_exact(A, b0):
    members = int(np.diff(A.indptr).max()) if A.shape[0] else 0
    assert np.array_equal(b0 * GRID, np.round(b0 * GRID)), 'a value is not a multiple of 1/16'
    top = float(np.abs(b0).max()) if b0.size else 0.0
    assert top * max(members, 1) * GRID < 2.0 ** 53, 'a sum could round'


def counts_sum(A, b, tables):
    """(ns, neg, pos) of 'sum' scores: ns = A b0; per table row t, S = A b0[t], neg += S <= ns, pos += S >= ns."""
    b0 = _zeroed(b)
    _assert_exact(A, b0)
    ns = np.asarray(A @ b0)
    neg = np.zeros(ns.shape)
    pos = np.zeros(ns.shape)
    for t in np.asarray(tables):
        s = np.asarray(A @ b0[t])
        neg += s <= ns
        pos += s >= ns
    return ns, neg, pos


def counts_sum_batched(a_dense, b, tables):
    """counts_sum of a SMALL dense membership in one product over all permutations (tens of thousands of them)."""
    a = np.asarray(a_dense, dtype=np.float64)
    b0 = _zeroed(b)
    _assert_exact(sp.csr_matrix(a), b0)
    ns = a @ b0
    s = np.matmul(a, b0[np.asarray(tables)])                             # [P, n, m]
    return ns, (s <= ns).sum(axis=0).astype(np.float64), (s >= ns).sum(axis=0).astype(np.float64)


def z_score(A, b):
    """oracle/safe_oracle.py: compute_neighborhood_score(..., 'z-score'), operation by operation, on sparse products."""
    with np.errstate(invalid='ignore', divide='ignore'):
        notnan = ~np.isnan(b)
        b0 = np.where(notnan, b, 0)
        score = np.asarray(A @ b0)
        cnt = np.asarray(A @ np.where(notnan, 1.0, 0.0))
        mean = np.divide(score, cnt)
        exx = np.divide(np.asarray(A @ np.power(b0, 2)), cnt)
        std = np.sqrt(exx - np.power(mean, 2))
        score = np.divide(mean, std)
        score[std == 0] = np.nan
        score[cnt < 3] = np.nan
    return score


def counts_z(A, b, tables):
    """(ns, neg, pos, unclear) of z-scores.  A permutation is clear for a cell unless |z - obs| <= 1e-9 max(1, |obs|) (NaN on
    either side: clear, and false both ways); clear permutations are counted, the others tallied in `unclear`."""
    b = np.asarray(b, dtype=np.float64)
    obs = z_score(A, b)
    neg = np.zeros(obs.shape)
    pos = np.zeros(obs.shape)
    unclear = np.zeros(obs.shape)
    with np.errstate(invalid='ignore'):
        for t in np.asarray(tables):
            z = z_score(A, b[t])
            clear = ~(np.abs(z - obs) <= 1e-9 * np.maximum(1.0, np.abs(obs)))
            neg += (z <= obs) & clear
            pos += (z >= obs) & clear
            unclear += ~clear
    return obs, neg, pos, unclear


def outputs(ns, neg, pos, num_permutations, sign, thr):
    """oracle/safe_oracle.py: pvalues_by_randomization from the counters on, and binarize."""
    counts_neg = np.array(neg, dtype=np.float64)
    counts_pos = np.array(pos, dtype=np.float64)
    idx = np.isnan(ns)
    counts_neg[idx] = np.nan
    counts_pos[idx] = np.nan
    pvalues_neg = counts_neg / num_permutations
    pvalues_pos = counts_pos / num_permutations
    with np.errstate(invalid='ignore', divide='ignore'):
        nes_pos = -np.log10(np.where(pvalues_pos == 0, 1 / num_permutations, pvalues_pos))
        nes_neg = -np.log10(np.where(pvalues_neg == 0, 1 / num_permutations, pvalues_neg))
    nes = nes_pos if sign == 'highest' else nes_neg if sign == 'lowest' else nes_pos - nes_neg
    ok = ~np.isnan(nes)
    nes_binary = np.zeros(nes.shape)
    nes_binary[ok] = np.abs(nes[ok]) > -np.log10(thr)
    return {'pvalues_neg': pvalues_neg, 'pvalues_pos': pvalues_pos, 'nes': nes, 'nes_binary': nes_binary,
            'num_neighborhoods_enriched': np.sum(nes_binary, axis=0)}


# ---------------------------------------------------------------------------------------------------- the inputs ----

def layout(n, seed):
    return np.random.default_rng(seed).uniform(size=(n, 2))


def _with_gaps(b, rng):
    n = b.shape[0]
    b[rng.uniform(size=b.shape) < 0.03] = np.nan
    b[rng.choice(n, n // 25, replace=False)] = np.nan
    return b


def dyadic(n, m, seed):
    """Multiples of 1/16, 3 % NaN cells, n // 25 rows without a value."""
    rng = np.random.default_rng(seed)
    return _with_gaps(np.round(rng.normal(size=(n, m)) * GRID) / GRID, rng)


def normal(n, m, seed):
    rng = np.random.default_rng(seed)
    return _with_gaps(rng.normal(size=(n, m)), rng)


def binary(n, m, seed, densities, nan_rows=True):
    """0/1 columns of the given densities (resized to m); n // 30 rows without a value unless nan_rows is False."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, m))
    for j, d in enumerate(np.resize(np.asarray(densities, dtype=np.float64), m)):
        b[:, j] = rng.uniform(size=n) < d
    if nan_rows:
        b[rng.choice(n, n // 30, replace=False)] = np.nan
    return b


def binary_supports(n, sizes, seed):
    """0/1 columns with exactly sizes[j] ones; a size of None: a random column of density 0.2."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, len(sizes)))
    for j, k in enumerate(sizes):
        if k is None:
            b[:, j] = rng.uniform(size=n) < 0.2
        else:
            b[rng.choice(n, k, replace=False), j] = 1.0
    return b


def hub_membership(n, biggest, seed):
    """Dense int64: row 0 has exactly `biggest` members, row 1 `biggest` - 1, rows 2 .. 5 between 2048 and `biggest`, row 6
    none, the rest below 40 (each node in its own neighborhood)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, n), dtype=np.int64)
    sizes = np.concatenate([[biggest, biggest - 1], rng.integers(2048, biggest + 1, size=4), [0], rng.integers(1, 40, size=n - 7)])
    for i, k in enumerate(sizes):
        if k:
            others = rng.choice(n - 1, int(k) - 1, replace=False)
            a[i, others + (others >= i)] = 1
            a[i, i] = 1
    assert np.array_equal(a.sum(axis=1), sizes)
    return a


def small_membership(n):
    """A fixed matrix for a handful of nodes: row 1 is empty (n >= 2), the last row holds every node (n >= 3)."""
    i, j = np.indices((n, n))
    a = (((3 * i + 5 * j) % 4 != 0) | (i == j)).astype(np.int64)
    if n >= 2:
        a[1] = 0
    if n >= 3:
        a[n - 1] = 1
    return a


# A permutation of a handful of rows often maps a small neighborhood onto itself, and the z-score of the same members in another
# order is a tie only up to rounding.  The z-score cases on at most nine nodes therefore use sparser fixed matrices (density 0.4,
# the diagonal, row 1 empty, no row of all nodes), drawn with the seeds below: chosen on the reference so that, with the values of
# small_case and the seeded stream of PERM_SEED, no scored neighborhood meets its own members again in any of the SMALL_PERMS
# permutations (tests/test_perm_limits_ref_cpu.py asserts it, and that scores exist).
Z_SMALL_SEEDS = {1: 0, 2: 0, 7: 5, 8: 2088, 9: 116}


def small_membership_z(n):
    rng = np.random.default_rng(Z_SMALL_SEEDS[n])
    a = (rng.uniform(size=(n, n)) < 0.4).astype(np.int64)
    a[np.arange(n), np.arange(n)] = 1
    if n >= 2:
        a[1] = 0
    return a


SATURATION_N = 12


def saturation_inputs():
    """(membership, 0/1 columns, dyadic columns) of the saturated-counter case: 12 nodes, row 1 empty, row 11 all nodes; three
    columns, the middle one constant over the population, so that every permutation ties on it."""
    rng = np.random.default_rng(65535)
    a = small_membership(SATURATION_N)
    bits = (rng.uniform(size=(SATURATION_N, 3)) < 0.4).astype(np.float64)
    bits[:, 1] = 1.0
    quant = np.round(rng.normal(size=(SATURATION_N, 3)) * GRID) / GRID
    quant[:, 1] = 2.5
    return a, bits, quant


def rotation_table(n, count, shift):
    """`count` rows of one fixed rotation (shift 0: the identity)."""
    return np.tile((np.arange(n, dtype=np.int64) + shift) % n, (count, 1))


# the z-score inputs of the GPU file: name -> (nodes, columns, permutations, radius, layout seed, value seed)
Z_LIMIT_CASES = {'lds_4549': (4549, 3, 12, 0.04, 4549, 71), 'lds_4550': (4550, 3, 12, 0.04, 4550, 72), 'n300': (300, 5, 33, 0.12, 300, 73)}
SMALL_NS = (1, 2, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025)
SMALL_PERMS = 33
SMALL_RADIUS = 0.12
PERM_SEED = 11
# the scatter kernel's prefetch queue over P: 1, 2 and both sides of every 16-permutation chunk; supports on both sides of the
# 256 rows its four waves take per round (None: a random column)
SWEEP_PERMS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
SWEEP_SUPPORTS = (0, 1, 64, 255, 256, 257, 300, None)
SWEEP_SEED = 100


def radius_for(n):
    return 0.012 if n >= 16000 else 0.04 if n >= 4000 else 0.12


def euclidean_csr(xy, r):
    """(indptr, indices) of A[i, j] = (|x_i - x_j| < r), row by row through a k-d tree: the host stand-in for
    Neighborhoods.euclidean where no device is at hand (the GPU tests read the device's own membership back)."""
    from scipy.spatial import cKDTree
    xy = np.asarray(xy, dtype=np.float64)
    tree = cKDTree(xy)
    rows = tree.query_ball_point(xy, r)
    cols = []
    for i, cand in enumerate(rows):
        cand = np.sort(np.asarray(cand, dtype=np.int64))
        d = np.sqrt(((xy[cand] - xy[i]) ** 2).sum(axis=1))
        cols.append(cand[d < r])
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    return indptr, (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int64)


def small_case(n, score, m):
    """(dense membership or None, layout or None, values) of a small-shape case of the LDS f64 kernel."""
    values = (normal if score == 'z-score' else dyadic)(n, m, 1000 * n + m)
    if score != 'z-score':
        values[0, 0] = 2.5                                               # (never a block of nothing but 0, 1 and NaN: that is 0/1 data)
    if n <= 9:
        return (small_membership_z if score == 'z-score' else small_membership)(n), None, values
    return None, layout(n, n), values
