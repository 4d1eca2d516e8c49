"""Designed inputs of the exact hypergeometric tests: every (pop, K, n, x) of a case is chosen, not drawn.

Node order: the `pop` nodes with a value first, then `n_nan` nodes whose attribute row is all NaN (they
leave the population, safe.py:574-588).  Neighborhood i = the first n_i nodes plus the first g_i NaN nodes
(members that count in the row sum of A but not in the neighborhood size); attribute j = ones on the nodes
[s_j, s_j + K_j).  So x_ij = |[0, n_i) & [s_j, s_j + K_j)| = clamp(n_i - s_j, 0, K_j), and a wanted x for a
pair (K, n) is the column s = n - x -- possible exactly when x lies in the support of Hypergeom(pop, K, n).

A case gives its distinct (n, g) pairs; the N rows cycle through them.  Columns are repeated when a call
would otherwise have too few elements per distinct (n, K) pair for the table forms (they need
4 * #sizes * #counts <= N * M, enrich.hip hypergeom_fused)."""
from fractions import Fraction

import numpy as np

import hyp_exact as hx

SMALLEST_NORMAL = Fraction(2.2250738585072014e-308)
# name -> (exclusive lower bound, inclusive upper bound) of the exact p; family 2 must populate each one
BANDS = {
    '1e-10': (Fraction(1, 10 ** 20), Fraction(1, 10 ** 10)),
    '1e-50': (Fraction(1, 10 ** 60), Fraction(1, 10 ** 50)),
    '1e-100': (Fraction(1, 10 ** 110), Fraction(1, 10 ** 100)),
    '1e-200': (Fraction(1, 10 ** 210), Fraction(1, 10 ** 200)),
    '1e-300': (SMALLEST_NORMAL * (1 - Fraction(1, 2 ** 60)), Fraction(1, 10 ** 300)),
    'subnormal': (Fraction(0), SMALLEST_NORMAL * (1 - Fraction(1, 2 ** 60))),
}
_BOUNDS = [Fraction(1, 10 ** e) for e in (10, 13, 16, 50, 53, 56, 100, 103, 106, 200, 203, 206, 300, 303, 306)] + [SMALLEST_NORMAL, Fraction(1, 10 ** 320)]


def band_of(e):
    for name, (low, high) in BANDS.items():
        if low < e <= high:
            return name
    return None


def targets(pop, K, n, deep=True):
    """The x worth a cell for one (K, n): both ends of the support and their neighbours, around the mean, points between the
    mean and the top, and (deep) the first x below each decade bound down to the subnormals."""
    lo, hi = hx.support(pop, K, n)
    mean = K * n // pop
    xs = {lo, lo + 1, mean - 1, mean, mean + 1, hi - 1, hi}
    xs.add((K + 1) * (n + 1) // (pop + 2))                      # the mode
    for num in (1, 2, 4, 6, 7):
        xs.add(mean + (hi - mean) * num // 8)
    if deep:
        for bound in _BOUNDS:
            x = hx.first_x_below(pop, K, n, bound)
            if x is not None:
                xs.add(x)
    return sorted(x for x in xs if lo <= x <= hi)


class Case:
    def __init__(self, name, family, pop, n_nan, sizes, cols, min_rows=0, extra_rows=()):
        self.name, self.family, self.pop, self.n_nan = name, family, pop, n_nan
        self.n_total = pop + n_nan
        sizes = list(dict.fromkeys(sizes))
        cols = list(dict.fromkeys(cols))
        assert all(0 <= n <= pop and 0 <= g <= n_nan for n, g in sizes), name
        assert all(0 <= K and 0 <= s and s + K <= pop for K, s in cols), name
        self.sizes = sizes
        # the rows cycle through the sizes; extra_rows = sizes that only ONE row has (the last ones: a hub)
        self.rows = [sizes[i % len(sizes)] for i in range(self.n_total - len(extra_rows))] + list(extra_rows)
        n_sizes = len(set(n for n, _ in self.rows))
        n_counts = len(set(K for K, _ in cols))
        reps = 1
        while self.n_total * len(cols) * reps < 4 * n_sizes * n_counts:
            reps += 1
        self.cols = cols * reps
        self.max_row_count = max(n + g for n, g in self.rows)
        # the count route of the table forms is the bit-sliced one: neighborhoods below 1024 members (enrich.hip counts_route)
        self.table_ok = self.max_row_count < 1024
        first, last = {}, {}
        for i, r in enumerate(self.rows):
            first.setdefault(r, i)
            last[r] = i
        self.checked_rows = sorted(set(first.values()) | set(last.values()))

    def __repr__(self):
        return self.name

    def arrays(self):
        n = self.n_total
        a = np.zeros((n, n), dtype=np.int64)
        for i, (ni, gi) in enumerate(self.rows):
            a[i, :ni] = 1
            a[i, self.pop:self.pop + gi] = 1
        b = np.zeros((n, len(self.cols)), dtype=np.float64)
        for j, (K, s) in enumerate(self.cols):
            b[s:s + K, j] = 1.0
        b[self.pop:, :] = np.nan
        return a, b

    def designed(self):
        """(K [M], n [rows], x [rows, M]) of the checked rows, from the design alone."""
        K = np.array([c[0] for c in self.cols], dtype=np.int64)
        s = np.array([c[1] for c in self.cols], dtype=np.int64)
        n = np.array([self.rows[i][0] for i in self.checked_rows], dtype=np.int64)
        x = np.clip(n[:, None] - s[None, :], 0, K[None, :])
        return K, n, x

    def recomputed(self, a, b):
        """The same from the arrays the library gets, the way the reference counts (safe.py:574-594)."""
        valid = ~np.isnan(b).all(axis=1) if b.shape[1] else np.ones(b.shape[0], dtype=bool)
        rows = a[self.checked_rows]
        n = rows @ valid.astype(np.int64)
        K = np.nansum(b, axis=0).astype(np.int64)
        x = np.rint(rows.astype(np.float64) @ np.nan_to_num(b)).astype(np.int64)
        return int(valid.sum()), K, n, x

    def triples(self):
        """The distinct (K, n, x) of the checked cells."""
        K, n, x = self.designed()
        kk = np.broadcast_to(K[None, :], x.shape)
        nn = np.broadcast_to(n[:, None], x.shape)
        return sorted(set(zip(kk.ravel().tolist(), nn.ravel().tolist(), x.ravel().tolist())))

    def expected(self):
        """{(K, n, x): exact tail} for the checked cells."""
        return {t: hx.exact_tail(self.pop, *t) for t in self.triples()}


def _all_intervals(pop):
    return [(0, 0)] + [(K, s) for K in range(1, pop + 1) for s in range(pop - K + 1)]


def family1():
    """Everything small: every reachable (K, n, x) of populations 1 .. 12, and 20 / 40 for p exactly 0.05."""
    cases = []
    for pop in range(1, 13):
        cols = _all_intervals(pop)
        cases.append(Case('small-N%d-sizes1toN' % pop, 1, pop, 0, [(n, 0) for n in range(1, pop + 1)], cols))
        cases.append(Case('small-N%d-sizes0toN-1' % pop, 1, pop, 0, [(n, 0) for n in range(pop)], cols))
    for pop in (3, 8, 11):                                      # one all-NaN row, a member of every other neighborhood
        cases.append(Case('small-N%d-one-nan-row' % (pop + 1), 1, pop, 1, [(n, n % 2) for n in range(pop + 1)], cols=_all_intervals(pop)))
    for pop in (20, 40):
        cases.append(Case('small-N%d' % pop, 1, pop, 0, [(n, 0) for n in range(1, pop + 1)], _all_intervals(pop)))
    return cases


def family1_padded():
    """The same populations inside a network of 320 nodes whose other rows are all NaN: every size 0 .. pop in one call, on a
    shape the matrix-core forms take."""
    cases = []
    for pop in list(range(1, 13)) + [20, 40]:
        sizes = [(n, g) for g in (0, 5) for n in range(pop + 1)]
        cases.append(Case('padded320-pop%d' % pop, 1, pop, 320 - pop, sizes, _all_intervals(pop)))
    return cases


def _grid(pop, ns, Ks, deep=True):
    cols = []
    for K in Ks:
        for n in ns:
            cols += [(K, n - x) for x in targets(pop, K, n, deep)]
    return cols


def family2():
    """Deep tails at ~2000 nodes."""
    cases = []
    pop = 2003                                                  # neither a multiple of 64 nor of 256
    small = [1, 2, 7, pop // 50, pop // 8, pop // 2]
    Ks = small + [pop - 3, pop]
    cases.append(Case('deep-N2003', 2, pop, 0, [(n, 0) for n in small], _grid(pop, small, Ks)))
    cases.append(Case('deep-N2003-large-neighborhoods', 2, pop, 0, [(n, 0) for n in small + [pop - 3, pop]],
                      _grid(pop, [pop // 2, pop - 3, pop], Ks)))
    pop = 2000                                                  # 40 all-NaN rows, some of them members
    small = [1, 2, 7, pop // 50, pop // 8, pop // 2]
    Ks = small + [pop - 3, pop]
    cases.append(Case('deep-N2040-40-nan-rows', 2, pop, 40, [(n, g) for n, g in zip(small, (0, 1, 40, 3, 0, 23))], _grid(pop, small, Ks)))
    pop = 1000                                                  # the whole network as a neighborhood, still on the table forms
    ns = [1, 2, 7, pop // 50, pop // 8, pop // 2, pop - 3, pop]
    cases.append(Case('deep-N1000', 2, pop, 0, [(n, 0) for n in ns], _grid(pop, ns, ns)))
    return cases


def family3():
    """Supports that start above 0: n + K - pop = 1, a few, pop / 2."""
    pop = 900
    ns = [450, 451, 455, 700, 899, 900]
    Ks = [451, 453, 650, 750, 899, 900, 1]
    return [Case('dense-N900', 3, pop, 0, [(n, 0) for n in ns], _grid(pop, ns, Ks, deep=False)),
            Case('dense-N930-30-nan-rows', 3, pop, 30, [(n, g) for n, g in zip(ns, (0, 30, 2, 0, 17, 1))],
                 _grid(pop, ns, Ks, deep=False))]


def family4():
    """The cut of the table at the call's largest count (split matrix-core form): the same columns in a call whose counts stay
    <= 2 under supports of hundreds, and in one where a cell sits at the top of a support of 300."""
    pop = 1000
    sizes = [(600, 0), (601, 0), (602, 0)]
    cols = [(K, s) for K in (3, 300, 390) for s in (600, 601, 602)] + [(50, 900)]       # (50, 900): every count 0
    # the largest count in the upper tail of supports that go on to 300 / 390: the terms beyond it are only summed, with an early exit
    tail = [(K, 600 - x) for K in (300, 390) for x in (200, 215, 225, 235)]
    return [Case('xmax-tiny', 4, pop, 0, sizes, cols),
            Case('xmax-top-of-support', 4, pop, 0, sizes + [(300, 0)], cols + [(300, 0)]),
            Case('xmax-in-the-tail', 4, pop, 0, sizes, tail)]


def family5():
    """Full size: 20 000 nodes."""
    pop = 20000
    ns = [1, 5, 60, 400, 1000, 1023]
    Ks = [1, 3, 40, 200, 2500, 10000, pop - 3, pop]
    cols, h = [], 0
    for K in Ks:
        for n in ns:
            xs = targets(pop, K, n)
            for pick in sorted({xs[h % len(xs)], xs[(h + len(xs) // 2) % len(xs)], xs[-1 - h % 3 if len(xs) > 3 else -1]}):
                cols.append((K, n - pick))
            h += 1
    cols = list(dict.fromkeys(cols))[:128]
    sizes = [(n, 0) for n in ns]
    return [Case('full-N20000', 5, pop, 0, sizes, cols),
            Case('full-N20000-hub', 5, pop, 0, sizes, cols, extra_rows=[(pop, 0)])]


def all_cases():
    return family1() + family1_padded() + family2() + family3() + family4() + family5()
