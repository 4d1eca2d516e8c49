"""multiple_testing_method on the host: statsmodels.stats.multitest.multipletests restated in NumPy, operation by operation, for
the five procedures of safepy_amd/csrc/fdr.hip -- the reference of tests/test_mt_ref_cpu.py, tests/test_gpu_mt.py,
tests/test_gpu_mt_api.py and tests/test_gpu_stream_procedures.py -- the count-form tables restated, and the designed families
that aim a procedure's running extreme at a chosen sorted rank.  Host only.

A family of `count` entries, ps the family sorted as np.argsort does (NaN last, the two zeros one value), k = 1 ... count:
  fdr_bh      raw = ps / (k / count);                 np.minimum.accumulate from the right; values above 1 become 1
  fdr_by      raw = ps / ((k / count) / c), c = np.sum(1. / np.arange(1, count + 1));       the same scan
  hochberg    raw = ps * np.arange(count, 0, -1);     the same scan
  holm        the same raw;                           np.maximum.accumulate from the left; values above 1 become 1
  bonferroni  p * float(count);                       values above 1 become 1
-0.0 is read as +0.0.  NaN: the minimum from the right carries one NaN (sorted last) through the whole family; the maximum from
the left and the element-wise product leave the numbers alone, which are then members of a family of `count` entries, NaNs
counted.  Every NaN that comes out is 0x7FF8...."""
import numpy as np

import fdr_cases as fc

METHODS = ('fdr_bh', 'fdr_by', 'holm', 'hochberg', 'bonferroni')
NUMBERS = {'fdr_bh': 0, 'fdr_by': 1, 'holm': 2, 'hochberg': 3, 'bonferroni': 4}      # SAFE_MT_*
POISONED = ('fdr_bh', 'fdr_by', 'hochberg')          # one NaN turns the whole family NaN
QNAN_BITS = 0x7FF8000000000000


def by_verbatim(count):
    """statsmodels' own expression (fdrcorrection, method 'n')."""
    return float(np.sum(1. / np.arange(1, count + 1)))


def rows(p, method, c_by=None):
    """Every row of p [n, count] as one family."""
    p = np.array(p, dtype=np.float64, ndmin=2)
    p = np.where(p == 0, 0.0, p)                                     # -0.0 is the value 0.0
    count = p.shape[1]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if method == 'bonferroni':
            out = p * float(count)
        else:
            order = np.argsort(p, axis=1, kind='stable')
            ps = np.take_along_axis(p, order, axis=1)
            k = np.arange(1, count + 1)
            if method == 'fdr_bh':
                raw = ps / (k / float(count))
            elif method == 'fdr_by':
                c = by_verbatim(count) if c_by is None else c_by
                raw = ps / ((k / float(count)) / c)
            else:
                assert method in ('holm', 'hochberg'), method
                raw = ps * np.arange(count, 0, -1)
            if method == 'holm':
                adj = np.maximum.accumulate(raw, axis=1)
            else:
                adj = np.minimum.accumulate(raw[:, ::-1], axis=1)[:, ::-1]
            out = np.empty_like(p)
            np.put_along_axis(out, order, adj, axis=1)
        out[out > 1] = 1
    out[np.isnan(out)] = np.nan                                      # one bit pattern
    assert (fc.bits(out)[np.isnan(out)] == QNAN_BITS).all()
    return out


def family(p, method, c_by=None):
    return rows(np.asarray(p, dtype=np.float64).reshape(1, -1), method, c_by)[0]


def adjust(p, scope, method, c_by=None):
    """p [n, m] along multiple_testing_scope: 'attributes' / 0 rows, 'neighborhoods' / 1 columns, 'all' / 2 the matrix."""
    p = np.asarray(p, dtype=np.float64)
    if scope in ('attributes', 0):
        return rows(p, method, c_by)
    if scope in ('neighborhoods', 1):
        return np.ascontiguousarray(rows(np.ascontiguousarray(p.T), method, c_by).T)
    assert scope in ('all', 2), scope
    return rows(p.reshape(1, -1), method, c_by).reshape(p.shape)


def family_size(shape, scope):
    return {'attributes': shape[1], 0: shape[1], 'neighborhoods': shape[0], 1: shape[0]}.get(scope, shape[0] * shape[1])


# ------------------------------------------------------------------------------------------------ the count forms ----

def count_table(hist, P, count, method, c_by=None):
    """The adjusted value per count c of a family of `count` entries p = c / P from its histogram (hist_to_table of fdr.hip):
    cum[c] = #entries with count <= c is the LAST sorted position of the tie at c, before[c] + 1 = cum[c] - hist[c] + 1 its FIRST.
    The running minimum from the right takes a tie's value at the last position, the running maximum from the left at the first."""
    hist = np.asarray(hist, dtype=np.int64)
    cum = np.cumsum(hist)
    before = cum - hist
    v = np.arange(P + 1) / float(P)
    with np.errstate(divide='ignore', invalid='ignore'):
        if method == 'holm':
            raw = np.where(hist > 0, (count - before) * v, -np.inf)
            adj = np.maximum.accumulate(raw)
        else:
            if method == 'fdr_bh':
                raw = v / (cum / float(count))
            elif method == 'fdr_by':
                raw = v / ((cum / float(count)) / (by_verbatim(count) if c_by is None else c_by))
            else:
                assert method == 'hochberg', method
                raw = (count - cum + 1) * v
            adj = np.minimum.accumulate(np.where(hist > 0, raw, np.inf)[::-1])[::-1]
    return np.where(adj > 1.0, 1.0, adj)


def counts_family(p, P, method, c_by=None):
    """One family of count ratios c / P through its histogram.  Under Holm the NaN entries stay out of the histogram and in the
    count; under the others one NaN makes everything NaN."""
    p = np.asarray(p, dtype=np.float64)
    flat = p.ravel()
    nan = np.isnan(flat)
    out = np.full(flat.shape, np.nan)
    if nan.any() and method in POISONED:
        return out.reshape(p.shape)
    cf = np.rint(flat[~nan] * float(P))
    assert ((cf >= 0) & (cf <= P) & (cf / float(P) == flat[~nan])).all()
    b = cf.astype(np.int64)
    out[~nan] = count_table(np.bincount(b, minlength=P + 1), P, flat.size, method, c_by)[b]
    return out.reshape(p.shape)


# --------------------------------------------------------------------------------------------- designed families ----

def chain(method, count, at):
    """p_(r), r = 0 ... count - 1, strictly increasing, whose raw values under `method` have ONE extreme, at rank `at`: the
    minimum for the procedures of the running minimum from the right (every rank <= at takes it), the maximum for Holm (every
    rank >= at takes it), so the value has to travel across every chunk on that side.
      fdr_bh, fdr_by  raw ~ 0.5 + 0.2 |x - x_at|, x = (r + 1) / count: fdr_cases._chain('min') (BY scales it by one constant)
      hochberg        p = (0.5 + 0.2 |x - x_at|) / (count - r): d p / d x > 0 because R count / (count - r) >= 0.25 > 0.2
      holm            p = (0.5 - 0.1 |x - x_at|) / (count - r): R >= 0.4, 0.4 count / (count + 1) >= 0.2 > 0.1
    Neighbouring raw values differ by >= 0.1 / count, far above the rounding of one product."""
    assert 0 <= at < count
    if method in ('fdr_bh', 'fdr_by', 'bonferroni'):
        return fc._chain('min', count, at)
    x = np.arange(1, count + 1) / float(count)
    raw = 0.5 + 0.2 * np.abs(x - x[at]) if method == 'hochberg' else 0.5 - 0.1 * np.abs(x - x[at])
    p = raw / np.arange(count, 0, -1)
    assert (np.diff(p) > 0).all()
    return p


def extreme_rank(p, method):
    """The sorted rank at which the raw values of the family have their extreme (what chain() aims)."""
    ps = np.sort(np.asarray(p, dtype=np.float64))
    count = ps.size
    k = np.arange(1, count + 1)
    raw = ps / (k / float(count)) if method in ('fdr_bh', 'fdr_by') else ps * np.arange(count, 0, -1)
    return int(np.argmax(raw) if method == 'holm' else np.argmin(raw))


def small(count, seed=0):
    """Uniform values scaled by 1 / count: the raw products (count - k + 1) p stay below 1, rise and fall again, and Holm
    (running maximum) and Hochberg (running minimum) differ in most entries -- swapping the scan direction cannot pass."""
    return np.random.default_rng([41, seed, count]).uniform(1e-6, 1.0, size=count) / float(count)


def clamp_family(count, seed=0):
    """Bonferroni / Holm / Hochberg products exactly 1, just below and just above: p = 1 / count and its neighbours, p = 1, and
    values whose product passes 1 by far."""
    rng = np.random.default_rng([43, seed, count])
    v = rng.uniform(1e-6, 1.0, size=count)
    one = 1.0 / count
    special = [one, np.nextafter(one, 0.0), np.nextafter(one, 1.0), 1.0, np.nextafter(1.0, 0.0), 0.5, 2.0, np.inf]
    k = min(count, len(special))
    v[rng.choice(count, k, replace=False)] = special[:k]
    return v


def tie_family(count, edges, seed=0):
    """Ascending values with tie groups of 5 equal entries straddling every sorted rank in `edges` (chunk and workgroup edges),
    shuffled."""
    rng = np.random.default_rng([47, seed, count])
    ps = np.sort(rng.uniform(1e-6, 1.0, size=count) / float(count) * 3.0)
    for e in edges:
        lo, hi = max(e - 2, 0), min(e + 3, count)
        if lo < hi:
            ps[lo:hi] = ps[lo]
    return rng.permutation(np.sort(ps))


def with_bits(v, at, pattern):
    v = np.array(v, dtype=np.float64)
    fc.bits(v)[at] = pattern
    return v


def designed_rows(method, m, form=None, seed=0):
    """((name, row), ...): fdr_cases.rows(m) -- uniform, ties, NaN of both signs first / middle / last, -0.0, subnormals, values
    above 1, the Benjamini-Hochberg chains -- then this procedure's own: its extreme in the chunks of fdr_cases.CHAIN_THREADS, the
    small family, the clamp family, tie groups across chunk edges, NaNs of both signs at both ends at once."""
    form = form or fc.default_form(m)
    out = list(fc.rows(m, seed, form))
    rng = np.random.default_rng([53, seed, m])
    perm = rng.permutation(m)
    if m >= 2:
        for t in fc.CHAIN_THREADS:
            at = fc.chain_rank(m, form, t)
            if at is not None:
                row = np.empty(m)
                row[perm] = chain(method, m, at)
                out.append(('mt_chain_t%d' % t, row))
    out.append(('small', small(m, seed)))
    out.append(('clamp', clamp_family(m, seed)))
    c = fc.chunk(m, form)
    out.append(('ties_at_chunk_edges', tie_family(m, [c, 2 * c, 127 * c, 255 * c], seed)))
    if m >= 4:
        row = small(m, seed + 1)
        row = with_bits(row, 0, fc.SIGN_NAN_BITS)
        row = with_bits(row, m // 2, fc.SIGN_NAN_BITS)
        row[m - 1] = np.nan
        row[1] = np.nan
        out.append(('nans_both_signs', row))
        row = small(m, seed + 2)
        row[m // 3], row[m // 2] = -0.0, 0.0
        out.append(('small_zeros', row))
    for _, row in out:
        assert row.shape == (m,) and row.dtype == np.float64
    return tuple(out)


_MATRICES = {}


def matrix(method, m, form=None):
    """(names, p [rows, m]) of designed_rows, cached and read-only."""
    key = (method if method in ('holm', 'hochberg') else 'bh', m, form)
    if key not in _MATRICES:
        named = designed_rows(key[0] if key[0] != 'bh' else 'fdr_bh', m, form)
        p = np.stack([row for _, row in named])
        p.setflags(write=False)
        _MATRICES[key] = (tuple(name for name, _ in named), p)
        if len(_MATRICES) > 6:
            _MATRICES.pop(next(iter(_MATRICES)))
    return _MATRICES[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(fc.bits(a), fc.bits(b))


def differing(names, got, want):
    return [name for name, g, w in zip(names, got, want) if not same_bits(g, w)]
