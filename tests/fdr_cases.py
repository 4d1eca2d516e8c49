"""Designed p-value rows, count matrices and the dispatch constants of safepy_amd/csrc/fdr.hip (chosen in fdr_plan.h; pinned to
what that header answers by tests/test_fdr_cases_cpu.py), shared by tests/test_fdr_cases_cpu.py and tests/test_gpu_fdr.py.
Host only.  The reference of everything built here is oracle.safe_oracle.fdrcorrection / fdr_rows (pinned to statsmodels on
the bits by tests/test_oracle_golden.py).

fdr.hip adjusts a row in one of three forms:
  block sort    k_fdr_row_sort<IPT>: 256 threads, thread t holds the sorted ranks [t IPT, (t + 1) IPT); rows of up to
                BLOCK_SORT_MAX attributes, IPT the smallest rung of IPT_LADDER with 256 IPT >= m.
  library sort  hipcub::DeviceSegmentedRadixSort + k_fdr_row: thread t takes the ranks [t len, (t + 1) len), len = ceil(m / 256);
                longer rows, or every row under SAFE_HIP_FDR_SORT=cub.
  histogram     k_fdr_row_counts: p-values that are counts / P with P <= HIST_MAX_P; thread t owns the bins
                [t per, (t + 1) per), per = ceil((P + 1) / 256).
In all three a thread takes the running minimum of its own chunk from the right, part[] carries the minima of the chunks to
the right of it.  The chain rows below decide where that minimum sits, so that it has to travel between chunks.

Everything returned is cached and read-only."""
import functools

import numpy as np

from oracle import safe_oracle as orc

THREADS = 256                               # fdr_plan.h: FDR_THREADS (part[], `t * IPT + i`, the parts of fdr_span)
IPT_LADDER = (4, 8, 12, 16, 20, 24, 28, 32)  # fdr_plan.h: FDR_IPT_LADDER, the rung chosen by fdr_row_form
BLOCK_SORT_MAX = 8192                       # fdr_plan.h: FDR_BLOCK_SORT_MAX = 256 * IPT_LADDER[-1]
HIST_BYTES_PER_BIN = 12                     # fdr_plan.h: FDR_ROW_HIST_BIN_BYTES (f64 table + u32 histogram)
HIST_LDS_BYTES = 60 * 1024                  # fdr_plan.h: FDR_ROW_HIST_LDS_BYTES
HIST_MAX_P = HIST_LDS_BYTES // HIST_BYTES_PER_BIN - 1      # 5119

CHAIN_THREADS = (0, 1, 127, 254, 255)       # the threads whose chunk gets the row's single minimum
SIGN_NAN_BITS = 0xFFF8000000000000          # what x86 makes of 0 / 0, inf - inf and log(-1)
ALL_ONES_BITS = 0xFFFFFFFFFFFFFFFF          # a NaN too; the bit pattern of the block sort's padding keys
HIST_P = (1, 2, 255, 256, 257, 5119, 5120)


def ipt_for(m):
    """The instantiation of k_fdr_row_sort that serves a row of m attributes; None: the library sort."""
    if m > BLOCK_SORT_MAX:
        return None
    need = -(-m // THREADS)
    return next(i for i in IPT_LADDER if need <= i)


def chunk(m, form):
    """Sorted ranks per thread: IPT (form 'block') or ceil(m / 256) (form 'library': fdr_plan.h, fdr_span over m)."""
    if form == 'block':
        assert ipt_for(m) is not None, m
        return ipt_for(m)
    assert form == 'library', form
    return -(-m // THREADS)


def default_form(m):
    return 'block' if m <= BLOCK_SORT_MAX else 'library'


def sort_lengths():
    """For every IPT the first length it serves and both sides of 256 IPT, where the sort has no padding keys; then 8193."""
    out = []
    for ipt in IPT_LADDER:
        out += [THREADS * (ipt - 4) + 1, THREADS * ipt - 1, THREADS * ipt]
    return out + [BLOCK_SORT_MAX + 1]


def library_lengths():
    """Under SAFE_HIP_FDR_SORT=cub: one thread with a chunk, len = 1 with and without idle threads, len = 2 with 127 idle
    threads (257), len = 33 with 7 (8193), len = 257 with a last chunk of 2 (65537)."""
    return [1, 2, 255, 256, 257, 8193, 65537]


def sort_id(m):
    """Case id of a row length under the default dispatch: the kernel that serves it."""
    ipt = ipt_for(m)
    return ('library' if ipt is None else 'ipt%d' % ipt) + '-m%d' % m


def hist_id(P):
    return 'P%d-%s' % (P, 'hist' if P <= HIST_MAX_P else 'sort')


def hist_bins(P, t):
    """The bins [b0, b1) of thread t in k_fdr_row_counts (fdr_plan.h: fdr_span over P + 1 bins and 256 parts)."""
    bins = P + 1
    per = -(-bins // THREADS)
    return min(t * per, bins), min(t * per + per, bins)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------- rows ----

def _chain(kind, m, at=None):
    """p_(r), r = 0 ... m - 1, strictly increasing, with raw_r = p_(r) / ((r + 1) / m):
      'up'    raw = 0.1 + 0.8 x, x = (r + 1) / m: strictly increasing, every entry keeps its own value;
      'down'  p = 0.25 + 0.5 x, raw = 0.25 / x + 0.5: strictly decreasing, every entry takes the last one's (0.75);
      'min'   raw = 0.5 + 0.2 |x - x_at|: one minimum at rank `at`; ranks <= at take it, the others keep theirs.
              (p = raw x has slope >= 0.5 - 2 * 0.2 > 0, so the ranks are the ones meant.)
    Neighbouring values differ by >= 0.1 / m, neighbouring raw values by >= 0.2 / m: far above the rounding of one division."""
    x = np.arange(1, m + 1) / float(m)
    if kind == 'up':
        return (0.1 + 0.8 * x) * x
    if kind == 'down':
        return 0.25 + 0.5 * x
    assert kind == 'min' and 0 <= at < m
    return (0.5 + 0.2 * np.abs(x - x[at])) * x


def chain_rank(m, form, t):
    """The rank in the middle of thread t's chunk of a row of m, or None where that thread has no rank."""
    c = chunk(m, form)
    if t * c >= m:
        return None
    return t * c + min(c // 2, m - 1 - t * c)


@functools.lru_cache(maxsize=None)
def rows(m, seed=0, form=None):
    """((name, row), ...): the designed rows of length m, only the kinds m is long enough for.  form: whose chunks the
    single-minimum rows aim at ('block' / 'library'; None: the form the default dispatch gives a row of m)."""
    form = form or default_form(m)
    rng = np.random.default_rng([seed, m])
    perm = rng.permutation(m)                                     # the fixed shuffle of the chain families

    def uniform():                                                # distinct values in (0, 1)
        u = rng.uniform(1e-6, 1.0, size=m)
        assert np.unique(u).size == m
        return u

    def with_bits(row, col, pattern):
        bits(row)[col] = pattern
        return row

    out = [('uniform', uniform())]
    if m >= 2:
        u = np.sort(uniform())
        out += [('ascending', u), ('descending', u[::-1].copy())]
    out.append(('ties40', rng.integers(0, 41, size=m) / 40.0))
    out.append(('ones', np.ones(m)))
    out.append(('one_value', np.full(m, 0.3)))
    for name, col, least in (('nan_first', 0, 1), ('nan_last', m - 1, 2), ('nan_middle', m // 2, 3)):
        if m >= least:
            row = uniform()
            row[col] = np.nan
            out.append((name, row))
    out.append(('all_nan', np.full(m, np.nan)))
    out.append(('sign_nan_middle', with_bits(uniform(), m // 2, SIGN_NAN_BITS)))
    out.append(('ones_bits_nan_middle', with_bits(uniform(), m // 2, ALL_ONES_BITS)))
    if m >= 2:
        row = uniform()
        row[m // 2] = -0.0
        out.append(('neg_zero', row))
    if m >= 3:
        row = uniform()
        row[m // 3], row[(2 * m) // 3] = -0.0, 0.0
        out.append(('both_zeros', row))
    tiny = np.array([5e-324, 1e-323, 2.5e-323, 1e-310, np.nextafter(2.2250738585072014e-308, 0.0), 2.2250738585072014e-308])
    row = uniform()
    k = min(m, tiny.size)
    row[rng.choice(m, k, replace=False)] = tiny[:k]
    out.append(('subnormal', row))
    if m >= 2:
        row = uniform() * 3.0
        row[m // 2] = np.inf
        assert (row > 1.0).sum() >= 1
        out.append(('above_one', row))
        for kind in ('up', 'down'):
            row = np.empty(m)
            row[perm] = _chain(kind, m)
            out.append(('chain_' + kind, row))
        for t in CHAIN_THREADS:
            at = chain_rank(m, form, t)
            if at is not None:
                row = np.empty(m)
                row[perm] = _chain('min', m, at)
                out.append(('chain_min_t%d' % t, row))
    for _, row in out:
        assert row.shape == (m,) and row.dtype == np.float64
        row.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def matrix(m, form=None, n=None):
    """(names, p): rows(m, seed, form) stacked; n: that many rows, taken from the seeds 0, 1, ... in turn."""
    names, stack, seed = [], [], 0
    while n is None or len(stack) < n:
        for name, row in rows(m, seed, form):
            names.append('%s/%d' % (name, seed))
            stack.append(row)
        seed += 1
        if n is None:
            break
    n = len(stack) if n is None else n
    p = np.stack(stack[:n])
    p.setflags(write=False)
    return tuple(names[:n]), p


@functools.lru_cache(maxsize=None)
def want(m, form=None, n=None):
    w = orc.fdr_rows(matrix(m, form, n)[1])
    w.setflags(write=False)
    return w


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def failing(names, got, wanted):
    """Names of the rows that differ (NaN equals NaN, -0.0 equals 0.0: the values statsmodels would compare)."""
    return [name for name, g, w in zip(names, got, wanted) if not same(g, w)]


# -------------------------------------------------------------------------------------------------------- counts ----

@functools.lru_cache(maxsize=None)
def count_rows(P, m, seed=0):
    """((name, counts), ...): rows of m permutation counts in [0, P] as f64 for the histogram form; one row carries a NaN, one a NaN with
    the sign bit set, one a -0.0 among positive counts."""
    rng = np.random.default_rng([seed, P, m])
    bins = P + 1
    last = (bins - 1) // (-(-bins // THREADS))                    # the last thread that owns a bin
    b0, b1 = hist_bins(P, last)
    assert b0 < b1 == bins and hist_bins(P, last + 1)[0] == bins
    out = [('zeros', np.zeros(m)), ('all_P', np.full(m, float(P))), ('middle', np.full(m, float((P + 1) // 2))),
           ('last_thread', rng.integers(b0, b1, size=m).astype(np.float64)),
           ('ties012', rng.integers(0, min(3, bins), size=m).astype(np.float64)),
           ('uniform', rng.integers(0, bins, size=m).astype(np.float64))]
    if m >= bins:
        row = np.concatenate([np.arange(bins), rng.integers(0, bins, size=m - bins)]).astype(np.float64)
        out.append(('every_count', rng.permutation(row)))
    row = rng.integers(0, bins, size=m).astype(np.float64)
    row[m // 2] = np.nan
    out.append(('one_nan', row))
    row = rng.integers(0, bins, size=m).astype(np.float64)
    bits(row)[m // 3] = SIGN_NAN_BITS
    out.append(('sign_nan', row))
    row = rng.integers(1, bins, size=m).astype(np.float64)
    row[(2 * m) // 3] = -0.0
    out.append(('neg_zero', row))
    for _, row in out:
        assert row.shape == (m,)
        row.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def count_matrix(P, m, seed=0):
    """(names, p): count_rows(P, m, seed) / P, the division NumPy does at safe.py:533-534."""
    named = count_rows(P, m, seed)
    counts = np.stack([row for _, row in named])
    p = counts / float(P)
    bits(p)[bits(counts) == SIGN_NAN_BITS] = SIGN_NAN_BITS      # (whatever the division makes of a NaN's sign)
    p.setflags(write=False)
    return tuple(name for name, _ in named), p


@functools.lru_cache(maxsize=None)
def count_want(P, m, seed=0):
    w = orc.fdr_rows(count_matrix(P, m, seed)[1])
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------------------------- the epilogue, k_nes_from_pvalues ----

THRESHOLD = 0.05
NES_N = (1, 63, 64, 65, 129)                # rows: the 64-row tile of a workgroup, walked by 4 rows per step
NES_M = (1, 63, 64, 65, 130)                # columns: the 64-column tile
NES_FORMS = ('hypergeometric', 'highest', 'lowest', 'both')
NES_PERM = 1000                             # num_permutations of the randomization forms
NES_MARGIN = 1e-9                           # 'both': the hit is |ep - en| > threshold on the device's log10 (see nes_case)
NES_SEED = 5


def nes_reference(form, p_neg, p_pos, num_permutations, threshold=THRESHOLD):
    """The adjusted p-values, nes, nes_binary and num_enriched of safe.py:536-554 / 599-608 + 468-472 from unadjusted
    p-values, all from the oracle's adjusted rows and the host's log10."""
    q_pos = orc.fdr_rows(p_pos)
    with np.errstate(invalid='ignore', divide='ignore'):
        if form == 'hypergeometric':
            q_neg, nes = None, -np.log10(q_pos)
        else:
            q_neg = orc.fdr_rows(p_neg)
            nes_pos = -np.log10(np.where(q_pos == 0, 1 / num_permutations, q_pos))
            nes_neg = -np.log10(np.where(q_neg == 0, 1 / num_permutations, q_neg))
            nes = {'highest': nes_pos, 'lowest': nes_neg, 'both': nes_pos - nes_neg}[form]
    nes_binary, num_enriched = orc.binarize(nes, threshold)
    return {'pvalues_neg': q_neg, 'pvalues_pos': q_pos, 'nes': nes, 'nes_binary': nes_binary, 'num_enriched': num_enriched}


def nes_margin(ref, threshold=THRESHOLD):
    """min | |nes| - (-log10 threshold) | over the cells that have a value."""
    nes = ref['nes'][~np.isnan(ref['nes'])]
    return np.abs(np.abs(nes) - -np.log10(threshold)).min() if nes.size else np.inf


@functools.lru_cache(maxsize=None)
def nes_case(form, n, m, seed=NES_SEED):
    """(p_neg or None, p_pos, num_permutations, reference): small p-values in most rows, so that cells stay enriched after
    the adjustment; with n >= 2, one NaN (its row comes out NaN and counts nowhere).  'highest' and 'lowest': count ratios
    c / NES_PERM with many zeros and ties (the histogram form runs first).  In the 'both' form the device decides on the
    difference of its own two log10, so no cell may be within NES_MARGIN of the threshold (the caller asserts it).  Count
    ratios cannot do that at any seed: adjusted values are c m / (k P), and pairs whose quotient is exactly 1 / 0.05 = 20
    (0 -> 0.001 against 0.02, 0.05 against 1) turn up in about 30 cells of 100 000.  So that form gets continuous values
    u^4 with exact zeros and ones mixed in, which reach the same epilogue through the sort; NES_SEED is a seed at which
    the margin holds at every shape of NES_N x NES_M."""
    rng = np.random.default_rng([seed, n, m])
    if form == 'hypergeometric':
        num_permutations, p_neg = 0, None
        p_pos = 10.0 ** -rng.uniform(0.0, 6.0, size=(n, m))
    else:
        num_permutations = NES_PERM
        if form == 'both':                                        # not count ratios: see the docstring
            p = rng.uniform(size=(2, n, m)) ** 4
            p[rng.uniform(size=p.shape) < 0.05] = 0.0             # (the 0 -> 1 / num_permutations rule)
            p[rng.uniform(size=p.shape) < 0.02] = 1.0
            p_neg, p_pos = p
        else:
            counts = np.floor(NES_PERM * rng.uniform(size=(2, n, m)) ** 4)
            counts[rng.uniform(size=counts.shape) < 0.02] = NES_PERM
            p_neg, p_pos = counts / float(NES_PERM)
    if n >= 2:
        for p in (p_neg, p_pos):
            if p is not None:
                p[n // 2, m // 2] = np.nan
    ref = nes_reference(form, p_neg, p_pos, num_permutations)
    for a in (p_neg, p_pos) + tuple(ref.values()):
        if a is not None:
            a.setflags(write=False)
    return p_neg, p_pos, num_permutations, ref


def boundary_values(threshold=THRESHOLD):
    """p-values around the binarisation boundary: the threshold and its two neighbours (-log10 maps all three to one double
    or not, as the host's libm decides: the reason nes_p_cut of common.h exists), then the largest double that the host's
    -log10(p) > -log10(threshold) still calls a hit and the one above it, wherever libm puts that pair."""
    thr = -np.log10(threshold)
    p = float(threshold)
    for _ in range(4096):
        if -np.log10(p) > thr:
            break
        p = np.nextafter(p, 0.0)
    for _ in range(4096):
        if not -np.log10(np.nextafter(p, 1.0)) > thr:
            break
        p = np.nextafter(p, 1.0)
    assert -np.log10(p) > thr and not -np.log10(np.nextafter(p, 1.0)) > thr
    return np.array([np.nextafter(threshold, 0.0), threshold, np.nextafter(threshold, 1.0), p, np.nextafter(p, 1.0)])
