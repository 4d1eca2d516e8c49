"""NumPy restatement of networkx 3.4.2's two Fruchterman-Reingold iterations (drawing/layout.py:
_fruchterman_reingold, f64 throughout, which spring_layout runs below 500 nodes, and _sparse_fruchterman_reingold, f32
positions / weights / k / t with an f64 displacement, which it runs from 500), and the seeded cases the layout tests
share.  Written from networkx's definition, not from layout.hip.  One iteration, for all rows at once:

  dx, dy   pos_i - pos_j for all pairs
  d        sqrt(dx*dx + dy*dy), d < 0.01 -> 0.01
  w        kk / (d*d) - (A*d) / k
  force    row i's ((term_0 + term_1) + ...) + term_{n-1} of dx*w, of dy*w: a strictly sequential sum in j (both of
           networkx's forms add in that order), here the last column of np.add.accumulate; widened to f64
  len      sqrt(fx*fx + fy*fy), len < 0.01 -> 0.1
  delta    f64 form: f * (t / len);  f32 form: (f * f64(t)) / len
  pos      dtype(f64(pos) + delta);  t -= dt;  stop once sqrt(sum(delta^2)) / n < threshold

In the f32 form A, pos, t and dt are f32, k is f32(k) and kk is f32(k*k) with the product taken in f64 (networkx
multiplies two Python floats before NumPy sees them).  tests/test_layout_ref_cpu.py holds fr_ref to the real functions
on the bits of the positions and on the iteration count, so the GPU tests (tests/test_gpu_layout_sweep.py) can sweep
sizes, densities and clamps that live networkx is too slow for: its f32 form costs ~190 us per row per iteration.

The only sum whose order is not networkx's is the one behind the stop decision (networkx: BLAS ddot of delta); the cases
that stop early put their threshold half a cooling step away from the nearest value that sum can take."""
import functools

import numpy as np

DMIN = 0.01                 # networkx's minimum distance
LEN_MIN, LEN_SET = 0.01, 0.1


def fr_ref(A_dense, k, pos0, iterations, threshold, dtype, stats=None, trace=None):
    """(positions [n,2] in dtype, iterations run).  stats, a dict, receives what the clamps did: 'd_clamped' = off-diagonal
    (i, j) with d < 0.01, summed over the iterations, 'd_zero' = those of them with d == 0, 'len_clamped' = rows with
    len < 0.01, summed likewise, 'first_clamped_pairs' / 'first_len_rows' = the sets of the first iteration, 'stop_margin' =
    the smallest |norm(delta) / n - threshold| / threshold any iteration saw (how far every stop decision was from
    depending on the order of that sum).  trace, a list, receives a copy of the positions after every iteration."""
    dtype = np.dtype(dtype)
    assert dtype in (np.dtype(np.float32), np.dtype(np.float64))
    f32 = dtype == np.dtype(np.float32)
    T = dtype.type
    A = np.asarray(A_dense, dtype=np.float64).astype(dtype)
    pos = np.asarray(pos0, dtype=np.float64).astype(dtype)
    n = pos.shape[0]
    assert A.shape == (n, n) and pos.shape == (n, 2)
    kt, kk, dmin = T(k), T(float(k) * float(k)), T(DMIN)
    t = T(max(pos[:, 0].max() - pos[:, 0].min(), pos[:, 1].max() - pos[:, 1].min())) * T(0.1)
    dt = T(t / T(iterations + 1))
    offdiag = ~np.eye(n, dtype=bool)
    if stats is not None:
        stats.update(d_clamped=0, d_zero=0, len_clamped=0, first_clamped_pairs=set(), first_len_rows=set(), stop_margin=np.inf)
    ran = 0
    for it in range(iterations):
        x, y = pos[:, 0], pos[:, 1]
        dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
        d = np.sqrt(dx * dx + dy * dy)
        low = d < dmin
        d = np.where(low, dmin, d)
        w = kk / (d * d) - (A * d) / kt
        assert w.dtype == dtype
        fx = np.add.accumulate(dx * w, axis=1)[:, -1].astype(np.float64)
        fy = np.add.accumulate(dy * w, axis=1)[:, -1].astype(np.float64)
        length = np.sqrt(fx * fx + fy * fy)
        short = length < LEN_MIN
        length = np.where(short, LEN_SET, length)
        if f32:
            px, py = (fx * np.float64(t)) / length, (fy * np.float64(t)) / length
        else:
            s = t / length
            px, py = fx * s, fy * s
        if stats is not None:
            hit = low & offdiag
            stats['d_clamped'] += int(hit.sum())
            stats['d_zero'] += int((hit & (dx == 0) & (dy == 0)).sum())
            stats['len_clamped'] += int(short.sum())
            if it == 0:
                stats['first_clamped_pairs'] = set(zip(*(v.tolist() for v in np.nonzero(hit))))
                stats['first_len_rows'] = set(np.flatnonzero(short).tolist())
        pos = np.stack([(x.astype(np.float64) + px).astype(dtype), (y.astype(np.float64) + py).astype(dtype)], axis=1)
        t = T(t - dt)
        ran = it + 1
        if trace is not None:
            trace.append(pos.copy())
        ratio = np.sqrt(float((px * px + py * py).sum())) / n
        if stats is not None and threshold > 0:
            stats['stop_margin'] = min(stats['stop_margin'], abs(ratio - threshold) / threshold)
        if ratio < threshold:
            break
    return pos, ran


# ---- the cases tests/test_layout_ref_cpu.py and tests/test_gpu_layout_sweep.py share -------------------------------------------

F32_BUDGET = 40000          # rows x iterations of an f32 case (the restatement is O(n^2) per iteration)


def csr_from_dense(A, keep=None):
    """(row_ptr, col, weight) of the entries of A that are nonzero or set in the boolean matrix keep (explicit zeros);
    columns strictly increasing."""
    mask = A != 0 if keep is None else ((A != 0) | keep)
    rows, cols = np.nonzero(mask)                            # row-major: columns increase within a row
    row_ptr = np.zeros(A.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=A.shape[0]), out=row_ptr[1:])
    return row_ptr, cols.astype(np.int32), A[rows, cols].astype(np.float64)


def random_adjacency(rng, n, p):
    """Symmetric, no self-loops, density p, weights uniform(0.5, 2): none of them survives rounding to f32."""
    upper = np.triu(rng.random_sample((n, n)) < p, 1)
    w = np.triu(rng.uniform(0.5, 2.0, size=(n, n)), 1)
    A = np.where(upper, w, 0.0)
    return A + A.T


def block_occupancy(row_ptr, col, rows=16, cols=128):
    """Entries per (16-row, 128-column) block of the CSR: the neighbour lists layout.hip scatters per (tile, chunk)."""
    n = row_ptr.shape[0] - 1
    r = np.repeat(np.arange(n), np.diff(row_ptr))
    occ = np.zeros(((n + rows - 1) // rows, (n + cols - 1) // cols), dtype=np.int64)
    np.add.at(occ, (r // rows, col // cols), 1)
    return occ


def make_case(name, n, dtype, p=None, iterations=100, k=0.2, threshold=1e-4, seed=None, A=None, pos0=None, keep=None,
              unit_weights=False, **extra):
    """A case: the CSR the device takes, the dense matrix it means, the start positions and the call's scalars."""
    seed = (n * 7919 + 17) % (2 ** 31) if seed is None else seed
    rng = np.random.RandomState(seed)
    pos = rng.rand(n, 2)                                     # pos0 = RandomState(seed).rand(n, 2)
    if A is None:
        A = random_adjacency(rng, n, min(1.0, 8.0 / n) if p is None else p)
    if unit_weights:
        A = (A != 0).astype(np.float64)
    if pos0 is not None:
        pos = np.array(pos0, dtype=np.float64)
    row_ptr, col, weight = csr_from_dense(A, keep)
    case = dict(name=name, n=n, dtype=np.dtype(dtype), A=A, row_ptr=row_ptr, col=col, weight=None if unit_weights else weight,
                pos0=pos, k=k, iterations=iterations, threshold=threshold)
    case.update(extra)
    return case


def f32_iterations(n, cap=100):
    """Iterations of an f32 case of n rows: within F32_BUDGET, and 10 from 2047 rows so that the restatement of one case
    stays near a second."""
    return max(1, min(cap, F32_BUDGET // n, 10 if n >= 2047 else cap))


SIZES_F64 = (1, 2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 255, 256, 257, 383, 384, 385, 496, 499)
SIZES_F32 = (500, 511, 512, 513, 527, 528, 639, 640, 641, 1023, 1024, 1025, 2047, 2048, 2049)


def size_cases():
    out = [make_case('f64-n%d' % n, n, np.float64) for n in SIZES_F64]
    out += [make_case('f32-n%d' % n, n, np.float32, iterations=f32_iterations(n)) for n in SIZES_F32]
    # the dtype is the caller's choice at the raw entry point: the f32 form with one and two chunks at full
    # iterations, the f64 form with five and nine
    out += [make_case('f32-n%d' % n, n, np.float32) for n in (16, 129, 256)]
    out += [make_case('f64-n%d' % n, n, np.float64, iterations=10) for n in (640, 1025)]
    return out


def dense_cases():
    return [make_case('dense-f64-n300-p0.6', 300, np.float64, p=0.6),
            make_case('dense-f64-n130-complete', 130, np.float64, p=1.0),
            make_case('dense-f32-n513-p0.5', 513, np.float32, p=0.5, iterations=10),
            make_case('dense-f32-n528-complete', 528, np.float32, p=1.0, iterations=10)]


def clamp_cases():
    """Start positions that reach `d < 0.01 -> 0.01` (coincident and near pairs; d exactly 0.01 and one ulp either side
    of it, which must and must not clamp) and `len < 0.01 -> 0.1` (zero net force), each in both dtypes.  'expect' says
    what fr_ref's stats have to show: pairs clamped / not clamped and rows with a short force in the first iteration."""
    out = []
    for dtype in (np.float64, np.float32):
        tag = 'f64' if dtype is np.float64 else 'f32'
        T = dtype
        # three coincident nodes: 0 and 1 with the same neighbours (they stay coincident throughout), 2 with others
        n = 24
        rng = np.random.RandomState(101)
        pos = rng.rand(n, 2)
        pos[1] = pos[2] = pos[0]
        A = random_adjacency(rng, n, 0.3)
        A[1] = A[0]
        A[:, 1] = A[:, 0]
        A[0, 0] = A[1, 1] = 0.0
        A[0, 1] = A[1, 0] = 1.25
        assert np.array_equal(A, A.T)
        out.append(make_case('clamp-coincident3-' + tag, n, dtype, A=A, pos0=pos,
                             expect=dict(clamped={(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)}, zero=True)))
        # a pair 0.005 apart, joined by an edge
        n = 17
        rng = np.random.RandomState(102)
        pos = rng.rand(n, 2)
        pos[5] = pos[11] + np.array([0.004, 0.003])
        A = random_adjacency(rng, n, 0.4)
        A[5, 11] = A[11, 5] = 0.75
        out.append(make_case('clamp-near-' + tag, n, dtype, A=A, pos0=pos, expect=dict(clamped={(5, 11), (11, 5)})))
        # d == 0.01 exactly and one ulp either side, in the form's own dtype: axis-aligned pairs from x = 0, so that
        # dx is the offset itself and sqrt(dx*dx + 0) returns it (a correctly rounded sqrt of a rounded square does)
        n = 33
        rng = np.random.RandomState(103)
        pos = 0.1 + 0.9 * rng.rand(n, 2)
        dmin = T(DMIN)
        below, above = np.nextafter(dmin, T(0)), np.nextafter(dmin, T(1))
        for a, b, off, yy in ((0, 1, dmin, 0.25), (2, 3, below, 0.5), (4, 5, above, 0.75)):
            pos[a] = (0.0, yy)
            pos[b] = (float(off), yy)
        A = random_adjacency(rng, n, 0.25)
        for a, b in ((0, 1), (2, 3), (4, 5)):
            A[a, b] = A[b, a] = 1.5
        out.append(make_case('clamp-ulp-' + tag, n, dtype, A=A, pos0=pos,
                             expect=dict(clamped={(2, 3), (3, 2)}, not_clamped={(0, 1), (1, 0), (4, 5), (5, 4)},
                                         distances={(0, 1): float(dmin), (2, 3): float(below), (4, 5): float(above)})))
        # zero net force: two coincident isolated nodes (t = 0 as well: it stops after one iteration) ...
        out.append(make_case('clamp-zero2-' + tag, 2, dtype, A=np.zeros((2, 2)), pos0=np.array([[0.375, 0.625]] * 2),
                             expect=dict(clamped={(0, 1), (1, 0)}, zero=True, short_rows={0, 1}, ran=1)))
        # ... and the centre of a symmetric cross with equal weights: its four terms cancel exactly
        pos = np.array([[0.5, 0.5], [0.75, 0.5], [0.25, 0.5], [0.5, 0.75], [0.5, 0.25]])
        A = np.zeros((5, 5))
        A[0, 1:] = A[1:, 0] = 1.5
        out.append(make_case('clamp-cross-' + tag, 5, dtype, A=A, pos0=pos, expect=dict(short_rows={0})))
    return out


def weight_cases():
    out = []
    for n, dtype in ((60, np.float64), (520, np.float32)):
        tag = 'f64-n60' if n == 60 else 'f32-n520'
        it = 100 if n == 60 else 20
        rng = np.random.RandomState(200 + n)
        base = random_adjacency(rng, n, 10.0 / n)
        edges = np.argwhere(np.triu(base, 1) != 0)
        # explicit zeros: a third of the edges are stored with weight 0
        A, keep = base.copy(), np.zeros((n, n), dtype=bool)
        for u, v in edges[::3]:
            A[u, v] = A[v, u] = 0.0
            keep[u, v] = keep[v, u] = True
        out.append(make_case('weights-zero-' + tag, n, dtype, A=A, keep=keep, iterations=it, stored_zeros=2 * len(edges[::3])))
        A = base.copy()
        for u, v in edges[::2]:
            A[u, v] = A[v, u] = -A[u, v]
        out.append(make_case('weights-negative-' + tag, n, dtype, A=A, iterations=it))
        A = base.copy()
        A[3, 3], A[n - 1, n - 1] = 2.5, 0.7
        out.append(make_case('weights-selfloop-' + tag, n, dtype, A=A, iterations=it))
        out.append(make_case('weights-none-' + tag, n, dtype, A=base, unit_weights=True, iterations=it))
    # weights that rounding to f32 changes by much less than uniform(0.5, 2) draws do: 1 + 2**-30 becomes 1
    n = 520
    rng = np.random.RandomState(777)
    A = (random_adjacency(rng, n, 10.0 / n) != 0) * (1.0 + 2.0 ** -30)
    out.append(make_case('weights-f32-rounding-f32-n520', n, np.float32, A=A, iterations=20))
    return out


def k_iteration_cases():
    out = []
    for k in (0.05, 0.2, 1.0 / 3.0, 1.0):
        out.append(make_case('k%.3g-f64-n129' % k, 129, np.float64, k=k, iterations=50))
        out.append(make_case('k%.3g-f32-n513' % k, 513, np.float32, k=k, iterations=20))
    for it in (1, 2, 3, 50, 101):
        out.append(make_case('it%d-f64-n129' % it, 129, np.float64, iterations=it))
        it = f32_iterations(513, it)                          # 101 -> 77: rows x iterations stays within F32_BUDGET
        out.append(make_case('it%d-f32-n513' % it, 513, np.float32, iterations=it))
    return out


def early_stop_cases():
    """While no row's force is short every node moves exactly t, so norm(delta) / n = t_it / sqrt(n) with
    t_it = t0 * (1 - it / (iterations + 1)).  A threshold halfway between t_{m-1} / sqrt(n) and t_m / sqrt(n) stops the run
    after m + 1 iterations, and sits half a cooling step (2.5 % of the value or more here) away from both: neither the f32
    rounding of t (1e-7) nor the order of the sum of squares (1e-16) comes near it."""
    out = []
    for n, dtype, iterations, stops in ((144, np.float64, 30, (11, 18)), (640, np.float32, 30, (11, 18))):
        tag = 'f64' if dtype is np.float64 else 'f32'
        for stop in stops:
            case = make_case('stop%d-%s-n%d' % (stop, tag, n), n, dtype, iterations=iterations)
            pos = case['pos0'].astype(dtype)
            t0 = float(max(pos[:, 0].max() - pos[:, 0].min(), pos[:, 1].max() - pos[:, 1].min())) * 0.1
            t_at = lambda it: t0 * (1.0 - it / (iterations + 1.0))          # noqa: E731
            case['threshold'] = 0.5 * (t_at(stop - 2) + t_at(stop - 1)) / np.sqrt(n)
            case['stop'] = stop
            out.append(case)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = size_cases() + dense_cases() + clamp_cases() + weight_cases() + k_iteration_cases() + early_stop_cases()
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return tuple(cases)


def case_named(name):
    return next(c for c in all_cases() if c['name'] == name)


_REFERENCE = {}


def reference(case):
    """(positions, iterations run, stats) of fr_ref for a case; computed once per process and returned read-only."""
    if case['name'] not in _REFERENCE:
        stats = {}
        pos, ran = fr_ref(case['A'], case['k'], case['pos0'], case['iterations'], case['threshold'], case['dtype'], stats=stats)
        pos.setflags(write=False)
        _REFERENCE[case['name']] = (pos, ran, stats)
    return _REFERENCE[case['name']]
