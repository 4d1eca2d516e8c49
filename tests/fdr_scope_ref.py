"""multiple_testing_scope on the host: the constants safepy_amd/csrc/fdr_plan.h chooses the column and whole-matrix forms of
fdr.hip by (pinned to what the header answers by tests/test_fdr_scope_cpu.py), NumPy restatements of the two count forms, and
the designed matrices shared by tests/test_fdr_scope_cpu.py, tests/test_gpu_fdr_scope.py and tests/test_gpu_fdr_scope_api.py.
The reference of everything is oracle.safe_oracle.fdrcorrection (pinned to statsmodels on the bits by
tests/test_oracle_golden.py): along axis 0 for the column scope, on the ravelled matrix for the whole-matrix scope.

fdr.hip adjusts
  a column   from its histogram over the counts (k_fdr_col_counts: a workgroup owns col_tile(P) adjacent columns, P <= COL_HIST_MAX_P),
             or as a row of the transposed matrix (k_fdr_transpose in TR_TILE x TR_TILE tiles, then the row forms);
  the matrix from one histogram (k_fdr_all_hist / _table / _map, P <= ALL_HIST_MAX_P), or from one sort: workgroup b of the
             suffix-minimum kernels owns the sorted ranks [b ALL_BLOCK, (b + 1) ALL_BLOCK), its thread t the ALL_IPT ranks from
             b ALL_BLOCK + t ALL_IPT on; k_fdr_all_carry joins the workgroups.
Host only; everything returned is read-only."""
import functools

import numpy as np

import fdr_cases as fc
from oracle import safe_oracle as orc

SCOPES = {'attributes': 0, 'neighborhoods': 1, 'all': 2}     # SAFE_FDR_SCOPE_ROWS / _COLS / _ALL

COL_LDS_BYTES = 128 * 1024                  # fdr_plan.h: FDR_COL_LDS_BYTES
COL_TILE_MAX = 16                           # FDR_COL_TILE_MAX
COL_TILE_MIN = 4                            # FDR_COL_TILE_MIN
COL_HIST_MAX_P = COL_LDS_BYTES // (8 * COL_TILE_MIN) - 1     # 4095
ALL_HIST_MAX_P = 64 * 1024 // 4 - 1         # 16383
TR_TILE = 32                                # FDR_TR_TILE
ALL_IPT = 8                                 # FDR_ALL_IPT
ALL_BLOCK = 256 * ALL_IPT                   # FDR_ALL_BLOCK


def col_tile(P):
    """Columns per workgroup of k_fdr_col_counts (fdr_plan.h: fdr_col_tile)."""
    return min(COL_TILE_MAX, COL_LDS_BYTES // (8 * (P + 1)))


# ------------------------------------------------------------------------------------------------ the references ----

def want(p, scope):
    """The host statement of the scope, from the oracle."""
    p = np.asarray(p, dtype=np.float64)
    if scope in ('attributes', 0):
        return orc.fdr_rows(p)
    if scope in ('neighborhoods', 1):
        return np.ascontiguousarray(orc.fdr_rows(np.ascontiguousarray(p.T)).T)
    assert scope in ('all', 2), scope
    return orc.fdrcorrection(p.ravel()).reshape(p.shape)


def _table(hist, P, count):
    """The adjusted value per count from one histogram: cum[c] is the last sorted position of the tie at c, raw[c] what
    statsmodels computes there (the same two divisions), then the running minimum from the right over the occupied bins."""
    cum = np.cumsum(hist)
    with np.errstate(divide='ignore', invalid='ignore'):
        raw = np.where(hist > 0, (np.arange(P + 1) / float(P)) / (cum / float(count)), np.inf)
    adj = np.minimum.accumulate(raw[::-1])[::-1]
    return np.where(adj > 1.0, 1.0, adj)


def _bins(p, P):
    """rint(p P), the bin rule of k_fdr_row_counts; the entries must be count ratios."""
    cf = np.rint(p * float(P))
    assert ((cf >= 0) & (cf <= P) & (cf / float(P) == p)).all()
    return cf.astype(np.int64)


def counts_cols(p, P):
    """The column count form restated: per column histogram -> table -> look-up; a column with a NaN becomes NaN."""
    p = np.asarray(p, dtype=np.float64)
    out = np.empty_like(p)
    for j in range(p.shape[1]):
        col = p[:, j]
        if np.isnan(col).any():
            out[:, j] = np.nan
            continue
        b = _bins(col, P)
        out[:, j] = _table(np.bincount(b, minlength=P + 1), P, col.size)[b]
    return out


def counts_all(p, P):
    """The whole-matrix count form restated: one histogram -> table -> look-up; a NaN anywhere makes everything NaN."""
    p = np.asarray(p, dtype=np.float64)
    if np.isnan(p).any():
        return np.full(p.shape, np.nan)
    b = _bins(p.ravel(), P)
    return _table(np.bincount(b, minlength=P + 1), P, p.size)[b].reshape(p.shape)


# --------------------------------------------------------------------------------------------- columns, sort form ----

COLS_SORT_N = (1, 2, 255, 256, 257, 1023, 1025, 4097, 8192, 8193) + (TR_TILE - 1, TR_TILE, TR_TILE + 1)
COLS_SORT_M = (1, 2, 63, 64, 65, 130) + (TR_TILE - 1, TR_TILE, TR_TILE + 1)


@functools.lru_cache(maxsize=4)
def cols_sort_matrix(n, m):
    """(names, p [n, m]): column j is the j-th designed row of fdr_cases.rows(n) (seeds in turn), transposed in."""
    names, cols, seed = [], [], 0
    while len(cols) < m:
        for name, row in fc.rows(n, seed):
            names.append('%s/%d' % (name, seed))
            cols.append(row)
        seed += 1
    p = np.ascontiguousarray(np.stack(cols[:m], axis=1))
    p.setflags(write=False)
    return tuple(names[:m]), p


# -------------------------------------------------------------------------------------------- columns, count form ----

COLS_COUNT_P = (1, 2, 255, 256, 257, COL_HIST_MAX_P, COL_HIST_MAX_P + 1)
COLS_COUNT_N = (1, 2, 257, 4099)


def cols_count_m(P):
    """Both sides of the column tile of P, and two full tiles and a part."""
    t = col_tile(min(P, COL_HIST_MAX_P))
    return (t - 1, t, t + 1, 2 * t + 1) if t > 1 else (1, 2, 3)


@functools.lru_cache(maxsize=8)
def cols_count_matrix(P, n, m):
    """(names, p [n, m]): column j is the j-th row of fdr_cases.count_matrix(P, n, seed), seeds in turn (NaN of both signs and
    -0.0 among them)."""
    names, cols, seed = [], [], 0
    while len(cols) < m:
        nm, mat = fc.count_matrix(P, n, seed)
        names += ['%s/%d' % (x, seed) for x in nm]
        cols += list(mat)
        seed += 1
    p = np.ascontiguousarray(np.stack(cols[:m], axis=1))
    p.setflags(write=False)
    return tuple(names[:m]), p


# ------------------------------------------------------------------------------------------------ the whole matrix ----

ALL_SHAPES = ((1, 1), (1, 2), (2, 1), (1, 257), (257, 1), (16, 16), (255, 257), (1000, 1031), (2049, 2051))
ALL_COUNT_P = (1, 257, 1000, ALL_HIST_MAX_P, ALL_HIST_MAX_P + 1)


def all_chain_positions(total):
    """{name: rank}: the middle of the first, a middle and the last thread chunk of the first, a middle and the last workgroup
    of k_fdr_all_blockmin / k_fdr_all_apply over `total` sorted ranks (fewer where the family is short)."""
    blocks = -(-total // ALL_BLOCK)
    out = {}
    for wname, b in (('first', 0), ('middle', blocks // 2), ('last', blocks - 1)):
        r0, r1 = b * ALL_BLOCK, min((b + 1) * ALL_BLOCK, total)
        chunks = -(-(r1 - r0) // ALL_IPT)
        for tname, t in (('first', 0), ('middle', chunks // 2), ('last', chunks - 1)):
            c0 = r0 + t * ALL_IPT
            at = c0 + min(ALL_IPT // 2, r1 - 1 - c0)
            out.setdefault(at, 'chain_min_wg-%s_chunk-%s' % (wname, tname))
    return {name: at for at, name in out.items()}


def all_sort_names(total):
    names = list(all_chain_positions(total)) if total >= 2 else []
    return names + ['nan_first', 'nan_middle', 'nan_last', 'above_one', 'one_value', 'ties40']


@functools.lru_cache(maxsize=2)
def _shuffle(total):
    return np.random.default_rng([11, total]).permutation(total)


def all_sort_family(shape, name):
    """The designed family `name` of length n m, reshaped: a chain with its single minimum at a chosen sorted rank (shuffled over
    the cells), a NaN at cell 0 / in the middle / at the last cell, values above 1 with +inf, one value, heavy ties."""
    total = shape[0] * shape[1]
    rng = np.random.default_rng([13, total])
    if name.startswith('chain_min'):
        v = np.empty(total)
        v[_shuffle(total)] = fc._chain('min', total, all_chain_positions(total)[name])
    elif name.startswith('nan_'):
        v = rng.uniform(1e-6, 1.0, size=total)
        v[{'nan_first': 0, 'nan_middle': total // 2, 'nan_last': total - 1}[name]] = np.nan
    elif name == 'above_one':
        v = rng.uniform(1e-6, 1.0, size=total) * 3.0
        v[total // 2] = np.inf
    elif name == 'one_value':
        v = np.full(total, 0.3)
    else:
        assert name == 'ties40', name
        v = rng.integers(0, 41, size=total) / 40.0
        v[total // 3] = -0.0
    return v.reshape(shape)


ALL_COUNT_NAMES = ('uniform', 'ties012', 'one_nan')


def all_count_family(shape, P, name):
    """Count ratios c / P of the whole-matrix count form: every count with a -0.0 among them, heavy ties on 0 / 1 / 2 with most
    entries zero, and a matrix with one NaN (sign bit set)."""
    total = shape[0] * shape[1]
    rng = np.random.default_rng([17, total, P])
    if name == 'ties012':
        c = rng.integers(0, min(3, P + 1), size=total).astype(np.float64)
        c[rng.uniform(size=total) < 0.7] = 0.0
    else:
        c = rng.integers(0, P + 1, size=total).astype(np.float64)
    p = c / float(P)
    if name == 'uniform':
        p[total // 3] = -0.0
    if name == 'one_nan':
        fc.bits(p)[total // 2] = fc.SIGN_NAN_BITS
    return p.reshape(shape)


# ----------------------------------------------------------------------------------------------------- by hand ----

# three answers for three scopes.  Rows: [.01 .04 .03 .02] / [.02 .5 .6 .04] / [.03 .9 .9 .9]
HAND_P = np.array([[0.01, 0.04, 0.03, 0.02], [0.02, 0.50, 0.60, 0.04], [0.03, 0.90, 0.90, 0.90]])
# rows (count 4): sorted .01 .02 .03 .04 -> raw .04 .04 .04 .04;  .02 .04 .5 .6 -> .08 .08 .6667 .6;  .03 .9 .9 .9 -> .12 1.2 .9 .9
HAND_ROWS = np.array([[0.01 / (1 / 4), 0.04 / (4 / 4), 0.03 / (3 / 4), 0.02 / (2 / 4)],
                      [0.02 / (1 / 4), 0.60 / (4 / 4), 0.60 / (4 / 4), 0.04 / (2 / 4)],
                      [0.03 / (1 / 4), 0.90 / (4 / 4), 0.90 / (4 / 4), 0.90 / (4 / 4)]])
# columns (count 3): .01 .02 .03 -> .03 .03 .03;  .04 .5 .9 -> .12 .75 .9;  .03 .6 .9 -> .09 .9 .9;  .02 .04 .9 -> .06 .06 .9
HAND_COLS = np.array([[0.01 / (1 / 3), 0.04 / (1 / 3), 0.03 / (1 / 3), 0.02 / (1 / 3)],
                      [0.03 / (3 / 3), 0.50 / (2 / 3), 0.90 / (3 / 3), 0.04 / (2 / 3)],
                      [0.03 / (3 / 3), 0.90 / (3 / 3), 0.90 / (3 / 3), 0.90 / (3 / 3)]])
# the matrix (count 12): sorted .01 .02 .02 .03 .03 .04 .04 .5 .6 .9 .9 .9 -> raw .12 (.12) .08 (.09) .072 (.08) .06857 .75 .8 (1.08) (.98) .9
# running minimum from the right: .06857 for every rank up to the second .04, then .75 .8 .9 .9 .9
HAND_ALL = np.array([[0.04 / (7 / 12)] * 4,
                     [0.04 / (7 / 12), 0.50 / (8 / 12), 0.60 / (9 / 12), 0.04 / (7 / 12)],
                     [0.04 / (7 / 12), 0.90 / (12 / 12), 0.90 / (12 / 12), 0.90 / (12 / 12)]])
