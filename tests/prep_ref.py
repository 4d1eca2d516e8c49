"""NumPy references and input builders for the layer under the enrichment kernels: the whole-matrix attribute facts of
attr.hip, the launch arithmetic and point sets of the fused dense Euclidean kernel, and designed membership matrices for the
derived forms of nbr.hip.  NumPy / SciPy only: nothing here touches the library.  Every comparison built on this module is
exact -- integers, bytes or f64 bit patterns."""
import numpy as np

# ------------------------------------------------------------------------------------------------ 1. attribute facts ----

NAN_ROWS = (0, 31, 32, 63, 64)                   # all-NaN rows of attr_input (and n - 1): both sides of the bitmap word edges
MIXED_VALUES = (0.0, 1.0, 2.0, -1.0, 0.5, -0.0, 1e30, np.inf, -np.inf)


# Fortran order takes the vector path of k_attr_stats: four packed rows per load, 1024 rows per wave of loads, 4096 per trip
F_SHAPES = tuple((n, m) for n in (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8195) for m in (1, 3)) + ((70, 130),)
# C order takes 64-column groups, 16 rows per trip, row chunks of max(256, a multiple of 64) rows: 17 chunks at n = 4097, the
# last of one row; m = 65 puts column 64 alone into a second group
C_SHAPES = tuple((n, m) for n in (1, 3, 16, 17, 255, 256, 257, 4097) for m in (2, 63, 64, 65, 130))
# the dynamic-LDS row bitmap: above 32 KiB from 262 145 rows on, and its documented ceiling of 150 KiB
LARGE_ROWS = (262144, 262209, 1228800)
LARGE_LAYOUTS = ((1, 'C'), (2, 'F'), (2, 'C'))
ROW_LIMIT = 1228800
# k_u8_to_f32 takes 16 bytes per thread (a workgroup: 256 x 16 = 4096) with a scalar tail: element counts and their shapes
U8_COUNTS = (1, 15, 16, 17, 4095, 4096, 4097, 256 * 16 - 1, 256 * 16 + 1)
U8_SHAPES = ((1, 1), (15, 1), (5, 3), (16, 1), (4, 4), (17, 1), (4095, 1), (1365, 3), (4096, 1), (64, 64), (4097, 1), (241, 17))


def attr_facts(b):
    """What the statistics pass, the census and the column sums must say about the node x attribute matrix b."""
    v = np.asarray(b).astype(np.float64)
    nan = np.isnan(v)
    val = ~nan
    with np.errstate(invalid='ignore'):
        non_integer = val & (v != np.floor(v))   # (+-inf is its own floor: an integer)
        col_sum = np.nansum(v, axis=0)           # (inf - inf inside a column: NaN -- the sums are compared on binary data only)
    row_flags = (~nan.all(axis=1)).astype(np.uint8)
    return {'n_other': int((val & (v != 0.0) & (v != 1.0)).sum()),
            'n_non_integer': int(non_integer.sum()),
            'max_nan_col': int(nan.sum(axis=0).max()),
            'row_flags': row_flags,
            'n_rows_with_value': int(row_flags.sum()),
            'value_counts': (int(nan.sum()), int((v == 0.0).sum()), int((v > 0.0).sum()), int((v < 0.0).sum())),
            'col_sum': col_sum}


def attr_design(n, m):
    """Where attr_input puts its designed rows: (all-NaN rows, row whose only value is in column m - 1 or None, row whose
    only value is in column 0 or None).  The single-value rows are the first two rows that are not all-NaN."""
    nan_rows = sorted({r for r in NAN_ROWS + (n - 1,) if r < n})
    free = [r for r in range(min(n, 70)) if r not in nan_rows]
    only_last = free[0] if len(free) > 0 else None
    only_first = free[1] if len(free) > 1 and m > 1 else None
    return nan_rows, only_last, only_first


def attr_input(n, m, dtype, flavour, seed, nan_column=False, designed=True):
    """A C-order [n, m] matrix of `dtype`.  flavour 'binary': 0 / 1; 'mixed': MIXED_VALUES; both with about 10 % NaN.
    Designed structure, each item wherever it fits the shape (attr_design): all-NaN rows at NAN_ROWS and n - 1, one row
    whose only value is in column m - 1 and one whose only value is in column 0, and the largest NaN count in the last
    column (raised until it is strictly the largest while rows are left).  nan_column: the last column is NaN throughout.
    uint8 / bool: 0 / 1 without NaN (the byte form has no missing values), no designed rows.  designed=False: the random
    part alone."""
    assert flavour in ('binary', 'mixed')
    rng = np.random.default_rng([seed, n, m, flavour == 'mixed'])
    dtype = np.dtype(dtype)
    if dtype.kind != 'f':
        assert flavour == 'binary'
        return (rng.uniform(size=(n, m)) < 0.3).astype(dtype)
    if flavour == 'binary':
        b = (rng.uniform(size=(n, m)) < 0.3).astype(np.float64)
    else:
        b = np.asarray(MIXED_VALUES)[rng.integers(0, len(MIXED_VALUES), size=(n, m))]
    b[rng.uniform(size=(n, m)) < 0.1] = np.nan
    if designed:
        nan_rows, only_last, only_first = attr_design(n, m)
        b[nan_rows] = np.nan
        if only_last is not None:
            b[only_last] = np.nan
            b[only_last, m - 1] = 1.0
        if only_first is not None:
            b[only_first] = np.nan
            b[only_first, 0] = 1.0
        if m > 1:
            free = ~np.isnan(b[:, m - 1])
            free[[r for r in (only_last, only_first) if r is not None]] = False
            room = np.nonzero(free)[0].tolist()
            counts = np.isnan(b).sum(axis=0)
            while room and counts[m - 1] <= counts[:m - 1].max():
                b[room.pop(), m - 1] = np.nan
                counts[m - 1] += 1
    if nan_column:
        b[:, m - 1] = np.nan
    return b.astype(dtype)


# ------------------------------------------------------------------------------- 2. the fused dense Euclidean kernel ----

DENSE_CHUNK_COLUMNS = 512                        # columns of a row one workgroup writes (256 lanes x 2)
DENSE_WORKGROUPS_PER_CU = 4
DENSE_BATCH = 8                                  # K1B_BATCH


def dense_geometry(n, num_cu):
    """The launch arithmetic of safe_euclidean_dense_dev: (chunks_per_row, rows_per_sweep, runs_whole_batches).  A
    workgroup starts at row i0 < rows_per_sweep and takes a whole batch while i0 + 7 rows_per_sweep < n."""
    chunks_per_row = -(-n // DENSE_CHUNK_COLUMNS)
    rows_per_sweep = max(1, min(n, DENSE_WORKGROUPS_PER_CU * num_cu // chunks_per_row))
    return chunks_per_row, rows_per_sweep, (DENSE_BATCH - 1) * rows_per_sweep < n


def first_batched_n(num_cu, limit=1 << 16):
    """The smallest n at which the kernel runs a whole batch (None: none below `limit`)."""
    for n in range(1, limit):
        if dense_geometry(n, num_cu)[2]:
            return n
    return None


DENSE_SLOTS = ('1', '2', '3', '511', '512', '513', '1024', '1025', 'nb-1', 'nb', 'nb+1', 'next_chunk_odd', 'next_chunk_even')


def dense_sizes(num_cu):
    """The sizes of the dense-kernel test for a device, by slot: the fixed edges, both sides of nb = the first n that runs
    whole batches, and the next odd and even n past the next change of chunks_per_row.  Returns (nb, {slot: n})."""
    nb = first_batched_n(num_cu)
    sizes = {s: int(s) for s in DENSE_SLOTS if s.isdigit()}
    if nb is not None:
        k = dense_geometry(nb + 1, num_cu)[0] * DENSE_CHUNK_COLUMNS + 1          # first n with one chunk more: odd
        sizes.update({'nb-1': nb - 1, 'nb': nb, 'nb+1': nb + 1, 'next_chunk_odd': k, 'next_chunk_even': k + 1})
    return nb, sizes


def last_lane_has_one_column(n):
    """The lane of column n - 1 holds a single column (`two == false` in k_euclid_dense): lanes own column pairs 2t, 2t + 1."""
    return n % 2 == 1


XY_KINDS = ('uniform', 'lattice', 'offset', 'huge', 'tiny')
# the designed threshold of a kind: a power of two, so that the pair (2, 3) of xy_input lies EXACTLY on it
XY_RADIUS = {'uniform': 0.125, 'lattice': 2.0, 'offset': 0.125, 'huge': 2.0 ** 500, 'tiny': 2.0 ** -530}


def xy_input(kind, n, seed=0):
    """Coordinates [n, 2].  Where n > 10: nodes 0 and 1 coincide, and nodes 2 and 3 are exactly XY_RADIUS[kind] apart (every
    operation of that distance is exact), so under the strict `<` they are NOT members of each other."""
    rng = np.random.default_rng([seed, n, XY_KINDS.index(kind)])
    u = rng.uniform(size=(n, 2))
    nr = XY_RADIUS[kind]
    if kind == 'uniform':
        xy, base = u, (0.25, 0.5)
    elif kind == 'lattice':                      # integer grid: many exact ties, distances exactly 1, 2, 5 (3-4-5), ...
        side = int(np.ceil(np.sqrt(n)))
        k = np.arange(n)
        xy, base = np.stack([k // side, k % side], axis=1).astype(np.float64), (7.0, 9.0)
    elif kind == 'offset':                       # differences cancel eleven digits
        xy, base = 1e6 + u, (1e6 + 0.25, 1e6 + 0.5)
    elif kind == 'huge':                         # squares overflow: every distance of two random nodes is +inf
        xy, base = u * 1e160, (2.0 ** 530, 2.0 ** 530)
    elif kind == 'tiny':                         # squares are subnormal
        xy, base = u * 1e-160, (2.0 ** -529, 2.0 ** -529)
    else:
        raise ValueError(kind)
    if n > 10:
        xy[1] = xy[0]
        xy[2] = base
        xy[3] = (base[0] + nr, base[1])
        assert xy[3, 0] - xy[2, 0] == nr and np.sqrt(nr * nr) == nr
    return xy


def separately_rounded_distances(xy):
    """sqrt(dx * dx + dy * dy) with every operation rounded on its own: the arithmetic the kernels restate."""
    x, y = xy[:, 0], xy[:, 1]
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    with np.errstate(over='ignore', under='ignore'):
        return np.sqrt(dx * dx + dy * dy)


def squared_threshold(nr):
    """The host rule of nbr.hip: T with  s < T  <=>  sqrt(s) < nr  for every s >= 0 (sqrt is correctly rounded and monotone)."""
    nr = np.float64(nr)
    if not nr > 0.0:
        return np.float64(0.0)
    if np.isinf(nr):
        return nr
    with np.errstate(over='ignore', under='ignore'):
        c = nr * nr
    if np.isinf(c):
        return c
    while c > 0.0 and np.sqrt(c) >= nr:
        c = np.nextafter(c, 0.0)
    while np.sqrt(c) < nr:
        c = np.nextafter(c, np.inf)
    return c


def radius_edges(xy):
    """The radii of the edge test: none, negative, NaN, everything, beyond every finite distance, below every subnormal
    square root, the smallest subnormal, and the reference's default 0.15 x the range of x."""
    span = float(xy[:, 0].max() - xy[:, 0].min())
    return (0.0, -1.0, np.nan, np.inf, 1e200, 1e-200, 5e-324, 0.15 * span)


def edge_input(n, n_edges, seed=0):
    """n_edges edges over n nodes; a self edge first and a repeated edge last, where they fit."""
    rng = np.random.default_rng([seed, n, n_edges])
    eu = rng.integers(0, n, size=n_edges).astype(np.int32)
    ev = rng.integers(0, n, size=n_edges).astype(np.int32)
    if n_edges >= 1:
        ev[0] = eu[0]
    if n_edges >= 3:
        eu[-1], ev[-1] = eu[1], ev[1]
    return eu, ev


# ------------------------------------------------------------------------------------------------ 3. membership forms ----

GROUP_COLUMNS = 4096                             # k_fill_csr / k_row_popcount walk a row in groups of 64 words


MEMBERSHIP_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4161)


def membership_design(n):
    """Designed rows of membership(n), each where it fits: {name: row}."""
    rows = {'full': 0}
    if n >= 2:
        rows['empty'] = 1
    if n >= 3:
        rows['only_last'] = 2
    if n > GROUP_COLUMNS and n >= 5:
        rows['beyond_group'] = 3                 # members only in columns >= 4096
        rows['straddle'] = 4                     # members exactly at 4095 and 4096
    return rows


def membership(n, seed=0):
    """int64 [n, n] 0 / 1: the designed rows of membership_design, the other rows random -- about 1 % from 1000 nodes on,
    20 % below (1 % of 64 columns is an empty row)."""
    rng = np.random.default_rng([seed, n])
    a = (rng.uniform(size=(n, n)) < (0.01 if n >= 1000 else 0.2)).astype(np.int64)
    rows = membership_design(n)
    a[rows['full']] = 1
    if 'empty' in rows:
        a[rows['empty']] = 0
    if 'only_last' in rows:
        a[rows['only_last']] = 0
        a[rows['only_last'], n - 1] = 1
    if 'beyond_group' in rows:
        a[rows['beyond_group'], :GROUP_COLUMNS] = 0
        a[rows['beyond_group'], GROUP_COLUMNS] = 1
        a[rows['beyond_group'], n - 1] = 1
        a[rows['straddle']] = 0
        a[rows['straddle'], GROUP_COLUMNS - 1:GROUP_COLUMNS + 1] = 1
    return a


def csr_of(a):
    """(row_ptr int32 [n + 1], col int32 [nnz]) of a dense 0 / 1 matrix, columns ascending inside every row."""
    row_ptr = np.concatenate([[0], np.cumsum(a.sum(axis=1))]).astype(np.int32)
    return row_ptr, np.nonzero(a)[1].astype(np.int32)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)
