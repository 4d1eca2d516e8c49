"""Reference of attribute_transform = 'rank' (safepy_amd/csrc/rank.hip), in NumPy, and the case list the CPU and the GPU tests
share.

keys(): the order-preserving 64-bit key of rank.hip's rank_key.  midranks(): (less + leq + 1) / 2 from chunk-wise sorted keys,
the way k_rank_sort / k_rank_emit count.  want(): what the kernel is pinned to,
scipy.stats.rankdata(method='average', axis=0, nan_policy='omit')."""
import functools

import numpy as np

NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN = np.uint64(0x8000000000000000)


def chunk():
    """T: the rows one workgroup sorts -- the implementation's, not a copy."""
    from safepy_amd import _lib
    return _lib.RANK_CHUNK


def keys(b):
    """uint64 keys of b (any float / integer dtype), same shape: unsigned order == IEEE order of the values widened to f64;
    -0.0 as +0.0; NaN = all ones."""
    v = np.asarray(b).astype(np.float64)
    v = np.where(v == 0.0, 0.0, v)                            # -0.0 -> +0.0
    bits = np.ascontiguousarray(v).view(np.uint64)
    k = np.where(bits >> np.uint64(63) != 0, ~bits, bits | SIGN)
    return np.where(np.isnan(v), NAN_KEY, k)


def midranks(b, t=None):
    """R f64, same shape as b: per column (less + leq + 1) * 0.5 with less / leq summed over the column's chunks of t sorted
    keys (padded with all-ones keys), NaN where b is NaN."""
    t = chunk() if t is None else t
    k = keys(b)
    n, m = k.shape
    out = np.full((n, m), np.nan)
    for j in range(m):
        col = k[:, j]
        both = np.zeros(n, dtype=np.int64)
        for r0 in range(0, n, t):
            part = np.full(t, NAN_KEY, dtype=np.uint64)
            part[:min(t, n - r0)] = col[r0:r0 + t]
            part.sort()
            both += np.searchsorted(part, col, side='left') + np.searchsorted(part, col, side='right')
        live = col != NAN_KEY
        out[live, j] = (both[live] + 1) * 0.5
    return out


def want(b):
    from scipy.stats import rankdata
    b = np.asarray(b)
    if b.shape[1] == 0:
        return np.empty(b.shape, dtype=np.float64)
    return np.asarray(rankdata(b, method='average', axis=0, nan_policy='omit'), dtype=np.float64)


def column_kinds(n, dtype=np.float64, t=None):
    """The designed columns at n rows as a dict name -> column of `dtype` (f64 or f32)."""
    t = chunk() if t is None else t
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 + n)
    tiny = np.finfo(dtype).smallest_subnormal                 # 5e-324 for f64
    inf = dtype.type(np.inf)
    cols = {}
    distinct = rng.permutation(n).astype(dtype) - dtype.type(n // 2) + dtype.type(0.25)
    cols['distinct'] = distinct
    cols['all_equal'] = np.full(n, 3.5, dtype=dtype)
    cols['zero_one'] = (rng.uniform(size=n) < 0.3).astype(dtype)          # ties of thousands straddle the chunk edges
    run = distinct.copy()                                                  # a run of equal values across every chunk boundary
    for edge in range(t, n, t):
        run[max(edge - 3, 0):edge + 3] = dtype.type(0.125)
    run[:min(2, n)] = dtype.type(0.125)                                    # ... and tied with the runs of the other chunks
    cols['run_on_edges'] = run
    cols['ascending'] = np.arange(n).astype(dtype)
    cols['descending'] = -np.arange(n).astype(dtype)
    z = np.where(rng.uniform(size=n) < 0.5, dtype.type(0.0), -dtype.type(0.0)).astype(dtype)
    z[rng.uniform(size=n) < 0.2] = dtype.type(-1.0)
    z[rng.uniform(size=n) < 0.2] = dtype.type(1.0)
    cols['signed_zeros'] = z
    e = rng.normal(size=n).astype(dtype)
    e[rng.uniform(size=n) < 0.25] = inf
    e[rng.uniform(size=n) < 0.25] = -inf
    cols['infinities'] = e
    sub = (rng.integers(-3, 4, size=n).astype(dtype) * tiny).astype(dtype)   # -3 .. 3 smallest subnormals, +-0.0 among them
    sub[rng.uniform(size=n) < 0.1] = np.finfo(dtype).tiny
    cols['subnormals'] = sub
    base = rng.choice(np.array([1.0, -1.0, 1e300 if dtype == np.float64 else 1e30, -3.5e-7], dtype=dtype), size=n)
    ulp = np.where(rng.uniform(size=n) < 0.5, base, np.nextafter(base, dtype.type(0)))
    cols['one_ulp_apart'] = ulp.astype(dtype)                 # a truncated key or a wrong flip of the negatives reorders these
    cols['all_nan'] = np.full(n, np.nan, dtype=dtype)
    single = np.full(n, np.nan, dtype=dtype)
    single[n // 3] = dtype.type(-2.0)
    cols['single_value'] = single
    for pct in (1, 50, 99):
        c = np.round(rng.normal(size=n), 1).astype(dtype)     # (rounded: ties)
        c[rng.uniform(size=n) < pct / 100.0] = np.nan
        cols['nan_%d' % pct] = c
    if dtype == np.float64:
        # equal after a narrowing to f32, distinct in f64
        cols['f32_colliders'] = 1.0 + rng.integers(0, 4, size=n) * 2.0 ** -40
    else:
        # f32 neighbours: equal after a narrowing to 16 bits, distinct as f32 (and as f64)
        cols['f16_colliders'] = (np.float32(1.0) + rng.integers(0, 4, size=n).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    return cols


@functools.lru_cache(maxsize=None)
def designed(n, dtype='float64', order='F', nan_row=True):
    """[n, #kinds] matrix of the designed columns (read-only), one whole row NaN when nan_row and n > 2."""
    cols = column_kinds(n, np.dtype(dtype))
    b = np.empty((n, len(cols)), dtype=np.dtype(dtype), order=order)
    for j, name in enumerate(cols):
        b[:, j] = cols[name]
    if nan_row and n > 2:
        b[n // 2, :] = np.nan
    b.flags.writeable = False
    return b


def tiled(n, m, dtype='float64', order='C'):
    """[n, m]: the designed columns repeated until m columns are filled, each repeat shifted by its column number."""
    src = designed(n, dtype, 'F')
    b = np.empty((n, m), dtype=src.dtype, order=order)
    for j in range(m):
        b[:, j] = src[:, j % src.shape[1]] + src.dtype.type(j // src.shape[1])
    return b


def shapes_n():
    t = chunk()
    return [1, 2, 3, 63, 64, 65, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 3 * t + 7]


@functools.lru_cache(maxsize=None)
def big():
    """70 001 x 3: distinct values, 0/1, rounded values with 10 % NaN."""
    n = 70001
    rng = np.random.default_rng(70001)
    b = np.empty((n, 3), order='F')
    b[:, 0] = rng.permutation(n) * 0.5 - 1000.0
    b[:, 1] = rng.uniform(size=n) < 0.5
    b[:, 2] = np.round(rng.normal(size=n), 2)
    b[rng.uniform(size=n) < 0.1, 2] = np.nan
    b.flags.writeable = False
    return b


@functools.lru_cache(maxsize=None)
def want_cached(name, *args):
    """want() of designed(*args) / big(), computed once per session and read-only."""
    r = want(big() if name == 'big' else designed(*args))
    r.flags.writeable = False
    return r


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
