"""safe_attr_column_moments, safe_moments_test and SAFE.compute_pvalues(how='analytic') on the device (include/safe_hip.h;
safepy_amd/csrc/moments.hip) against tests/moments_ref.py: Fractions for the moments and z^2, mpmath at 50 digits for the root
and erfc.  Needs an MI355X.

Constants of moments.hip the shapes are chosen around: k_col_moments takes MOM_ROW_CHUNK = 2048 rows per block (64 columns x 4
row lanes in C order, one column x 256 threads otherwise); k_moments_emit takes MOM_ROW_TILE = 16 rows x MOM_COL_CHUNK = 1024
columns per block, a wave's 64 lanes on adjacent columns.

T1  column moments.  Integer inputs with |b| <= 1024 and an exact mean (n_v a power of two, or column sum a multiple of n_v):
    mean and css bit-equal to the rationals.  Real data: mean bit-equal to column_sums() / n_v in f64; css within
    (n_v + 4) 2^-53 relative of the exact sum of (b - mean_dev)^2 (two roundings per term and at most n_v - 1 from any
    summation order).  Constant columns exactly 0.  Two calls bit-equal.
T2  z against the exact z of the device's own ns, mean, css and the host's k_i.  The device rounds, in this order,
        f = (k (n_v - k)) / (n_v (n_v - 1))   [both products exact integers; the division rounds]
        var = f * Q;  sd = sqrt(var);  t = k * mu;  d = x - t;  z = d / sd
    Six operations can round: the division in f, f * Q, the root, k * mu, the subtraction and the last division.  The
    rounding of k * mu shifts d by at most 2^-53 |k mu|, that is z by 2^-53 |k mu| / sd: the cancellation in x - k mu.  Each of
    the other five moves z by at most 2^-53 |z| (the root halves what f and var carry; that is not credited).  Counting all
    six at 2^-53 |z|, and the cancellation term twice to cover the relative errors of sd that multiply it,
        |dz| <= 2^-53 (C_OPS |z| + 2 |k mu| / sd),  C_OPS = 6.
    ns is bit-equal to safe_score's.
T3  p-values against mpmath's erfc(z_dev / sqrt 2) / 2 at the device's z bits: relative error of the small side at most
    2 K_ref (1 + z^2) 2^-53 for |z| <= 37.5 (K_ref: what scipy.special.ndtr measures against mpmath on the designed z list,
    tests/test_moments_ref_cpu.py); beyond, the small side in [0, 2.3e-308] and the large side exactly 1; everywhere the large
    side bit-equal to 1 - small; degenerate cells exactly (1, 1, z = 0).
T4  nes against -log10 of the device's own p-values (rtol 1e-6, atol 1e-9, infinities equal); nes_binary and num_enriched exact
    given the device's p / nes for the three signs and thresholds 0.05 and 1e-9; z_dev = NULL changes no other output.
T5  SAFE.compute_pvalues(how='analytic').  T6  refusals, a busy caller stream, live allocations.
The worst errors seen are printed per bucket of |z| (pytest -s)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import moments_ref as mr

pytestmark = pytest.mark.gpu

ROW_CHUNK, ROW_TILE, COL_CHUNK, LANES = 2048, 16, 1024, 64     # MOM_ROW_CHUNK, MOM_ROW_TILE, MOM_COL_CHUNK of moments.hip, a wave
C_OPS = 6
OUTPUTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'num_enriched')
BUCKETS = (0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 24.0, 32.0, mr.Z_EDGE)
WORST_P = {}                                                    # bucket -> worst p error in units of (1 + z^2) 2^-53
WORST_Z = [0.0]                                                 # worst |dz| as a share of its bound
POISON = -12345.678


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


@pytest.fixture(scope='module')
def k_ref():
    k = mr.designed_k_ref()
    print('K_ref = %.3f' % k)
    assert np.isfinite(k) and 0 < k < 16
    return k


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_moments(be, ctx, nbr, attr, sign='both', thr=0.05, col0=0, col1=None, want_z=True, guard=64):
    """One safe_moments_test call on poisoned buffers that are `guard` doubles longer than needed: {name: array}."""
    n, m = attr.n, (attr.m if col1 is None else col1) - col0
    names = OUTPUTS + (('z',) if want_z else ())
    sizes = [n * m] * 5 + [m] + ([n * m] if want_z else [])
    bufs = [ctx.alloc_f64(s + guard) for s in sizes]
    poison = np.full(max(sizes) + guard, POISON)
    try:
        for b, s in zip(bufs, sizes):
            b.upload(poison[:s + guard])
        be.moments_test(ctx, nbr, attr, sign, thr, [b.ptr for b in bufs[:6]], col0, col1, z_ptr=bufs[6].ptr if want_z else None)
        assert ctx.last_kernel()[0] == 'k_moments_emit'
        out = {}
        for name, b, s in zip(names, bufs, sizes):
            flat = b.download((s + guard,))
            assert (flat[s:] == POISON).all(), '%s: the call wrote past the end of its output' % name
            out[name] = flat[:s].reshape((m,) if name == 'num_enriched' else (n, m)).copy()
            assert not (out[name] == POISON).any(), '%s: a cell was left unwritten' % name
    finally:
        for b in bufs:
            b.free()
    return out


def observed_scores(be, ctx, nbr, attr, col0=0, col1=None):
    n, m = attr.n, (attr.m if col1 is None else col1) - col0
    buf = ctx.alloc_f64(n * m)
    try:
        be.score(ctx, nbr, attr, 'sum', buf.ptr, col0, col1)
        return buf.download((n, m))
    finally:
        buf.free()


def check_cells(out, k, n_v, mean, css, k_ref, what):
    """T2 and T3 on every cell: cells with the same (ns, k, column) must agree bit for bit and one of them is checked exactly."""
    ns, z, pp, pn = out['ns'], out['z'], out['pvalues_pos'], out['pvalues_neg']
    n, m = ns.shape
    kk, jj = np.broadcast_to(np.asarray(k)[:, None], (n, m)), np.broadcast_to(np.arange(m)[None, :], (n, m))
    keys = np.stack([bits(ns).ravel().view(np.int64), kk.ravel(), jj.ravel()], axis=1)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.ravel()
    for name in ('z', 'pvalues_pos', 'pvalues_neg'):
        flat = bits(out[name]).ravel()
        assert np.array_equal(flat, flat[first][inverse]), '%s: %s differs between cells with the same ns, k and column' % (what, name)
    degenerate = np.zeros(len(first), dtype=bool)
    for u, at in enumerate(first):
        i, j = divmod(int(at), m)
        z_exact, sd, kmu = mr.exact_z(ns[i, j], k[i], n_v, mean[j], css[j])
        if z_exact is None:
            degenerate[u] = True
            assert (z[i, j], pp[i, j], pn[i, j]) == (0.0, 1.0, 1.0), '%s: degenerate cell (%d, %d) gives %r' % (what, i, j, (z[i, j], pp[i, j], pn[i, j]))
            continue
        bound = mr.U * (C_OPS * abs(z_exact) + 2 * abs(kmu) / sd)
        dz = abs(mr.MP.mpf(float(z[i, j])) - z_exact)
        WORST_Z[0] = max(WORST_Z[0], float(dz / bound) if bound > 0 else 0.0)
        assert dz <= bound, '%s: z(%d, %d) = %r, exact %s: off by %s, bound %s' % (what, i, j, z[i, j], mr.MP.nstr(z_exact, 20), mr.MP.nstr(dz, 5), mr.MP.nstr(bound, 5))
    live = ~degenerate[inverse].reshape(n, m)
    # the large side is 1 - the small side, in f64, everywhere
    upper = z >= 0
    small, large = np.where(upper, pp, pn), np.where(upper, pn, pp)
    assert np.array_equal(bits(large)[live], bits(1.0 - small)[live]), '%s: the large side is not 1 - the small side' % what
    assert (small[live] <= 0.5).all() and (small[live] >= 0).all() and not np.isnan(z).any(), what
    zs, where = np.unique(bits(z)[live], return_index=True)
    small_of = small[live][where]
    for zb, p in zip(zs.view(np.float64), small_of):            # (same z bits, same p bits: asserted above through the keys)
        zf, p = float(zb), float(p)
        if abs(zf) > mr.Z_EDGE:
            assert 0.0 <= p <= mr.SMALL_MAX, '%s: z = %r gives a small side of %r' % (what, zf, p)
            continue
        want = mr.small_side(zf)
        err = float(abs(mr.MP.mpf(p) - want) / want / ((1 + mr.MP.mpf(zf) ** 2) * mr.U))
        bucket = max(b for b in BUCKETS if b <= abs(zf))
        WORST_P[bucket] = max(WORST_P.get(bucket, 0.0), err)
        assert err <= 2 * k_ref, '%s: p(z = %r) = %r, exact %s: %.2f (1 + z^2) 2^-53, bound %.2f' % (what, zf, p, mr.MP.nstr(want, 20), err, 2 * k_ref)
    beyond = live & (np.abs(z) > mr.Z_EDGE)
    assert (large[beyond] == 1.0).all(), '%s: a large side beyond |z| = 37.5 is not 1' % what
    return int(degenerate.sum()), len(first)


def check_outputs(out, sign, thr, what):
    """T4: nes, nes_binary and the counts from the device's own p-values."""
    pp, pn, nes = out['pvalues_pos'], out['pvalues_neg'], out['nes']
    want = mr.nes_of(pp, pn, sign)
    assert not np.isnan(nes).any() and np.array_equal(np.isinf(nes), np.isinf(want)), what
    np.testing.assert_allclose(nes, want, rtol=1e-6, atol=1e-9, err_msg=what)
    assert np.array_equal(out['nes_binary'], mr.decisions(pp, pn, nes, sign, thr)), what
    assert np.array_equal(out['num_enriched'], out['nes_binary'].sum(axis=0)), what


def handles(be, ctx, case, dtype=np.float64, order='C'):
    b = case.b.astype(dtype) if dtype != np.uint8 else np.nan_to_num(case.b).astype(np.uint8)
    return be.Neighborhoods.from_dense(ctx, case.a), be.Attributes.from_host(ctx, np.asarray(b, order=order))


# ----------------------------------------------------------------------------------------------------------------- T1 ----

def paired_columns(n, m, dtype, seed):
    """Integer columns whose mean and css are exact whatever n is: a constant c in 1 .. 5 with p rows at c + 1 and p rows at
    c - 1 (mean c, css 2 p).  Float inputs also get rows without a value and, where c - 1 = 0, NaN cells in place of zeros."""
    rng = np.random.default_rng(seed)
    valid = np.ones(n, dtype=bool)
    if dtype != np.uint8 and n >= 8:
        valid[rng.choice(n, n // 8, replace=False)] = False
    rows = np.nonzero(valid)[0]
    b = np.zeros((n, m))
    mean, css = np.zeros(m), np.zeros(m)
    for j in range(m):
        c, p = j % 5 + 1, int(rng.integers(0, len(rows) // 2 + 1))
        pick = rng.permutation(rows)[:2 * p]
        b[:, j] = c
        b[pick[:p], j] += 1
        b[pick[p:], j] -= 1
        if dtype != np.uint8 and c == 1 and m > 1:              # (column 1 keeps every such row in the population)
            b[pick[p:][::2], j] = np.nan                         # a NaN cell counts as the 0 it replaces
        mean[j], css[j] = c, 2 * p
    if dtype != np.uint8:
        b[~valid] = np.nan
    return b, mean, css


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32, np.uint8])
def test_t1_integer_columns_are_exact(be, ctx, dtype, order):
    # rows: one, two, and the row chunk of k_col_moments on both sides; columns: one, and the 64-column group on both sides
    for n, m in ((1, 1), (2, 63), (ROW_CHUNK - 1, 64), (ROW_CHUNK, 65), (ROW_CHUNK + 1, 130), (2 * ROW_CHUNK + 1, 3)):
        b, mean, css = paired_columns(n, m, dtype, 11 * n + m)
        host = np.asarray(b.astype(dtype) if dtype != np.uint8 else b.astype(np.uint8), order=order)
        attr = be.Attributes.from_host(ctx, host)
        try:
            got = attr.column_moments()
            assert np.array_equal(bits(got[0]), bits(mean)) and np.array_equal(bits(got[1]), bits(css)), (n, m)
            again = attr.column_moments()
            assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(bits(again[1]), bits(got[1])), (n, m)
            if m > 4:                                            # a sub-range that starts past column 0
                part = attr.column_moments(3, m - 1)
                assert np.array_equal(bits(part[0]), bits(mean[3:m - 1])) and np.array_equal(bits(part[1]), bits(css[3:m - 1])), (n, m)
        finally:
            attr.close()


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_t1_designed_columns_are_exact(be, ctx, dtype, order):
    case = mr.designed()[0]
    attr = be.Attributes.from_host(ctx, np.asarray(case.b.astype(dtype), order=order))
    try:
        mean, css = attr.column_moments()
        assert attr.stats()['n_rows_with_value'] == case.n_v
        assert np.array_equal(bits(mean), bits([float(v) for v in case.mu]))
        assert np.array_equal(bits(css), bits([float(v) for v in case.q]))
    finally:
        attr.close()


@pytest.mark.parametrize('order', ['C', 'F'])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_t1_real_columns(be, ctx, dtype, order):
    rng = np.random.default_rng(5)
    n, m = 2 * ROW_CHUNK + 4, 6
    b = (rng.normal(size=(n, m)) * np.array([1, 1e-3, 1e3, 1, 1, 1]) + np.array([0, 5, 0, 1e4, 0, 0])).astype(dtype)
    b[rng.uniform(size=(n, m)) < 0.02] = np.nan                 # NaN cells
    b[rng.choice(n, 300, replace=False)] = np.nan               # rows without a value
    flags = mr.row_flags(b[:, :4])
    b[:, 4] = np.where(flags, dtype(0.1), np.nan)               # constant over the population, and no exact mean
    b[:, 5] = np.where(flags, -7, np.nan)
    assert np.array_equal(mr.row_flags(b), flags)
    attr = be.Attributes.from_host(ctx, np.asarray(b, order=order))
    try:
        n_v = int(flags.sum())
        assert attr.stats()['n_rows_with_value'] == n_v
        mean, css = attr.column_moments()
        assert np.array_equal(bits(mean), bits(attr.column_sums() / n_v))
        assert css[4] == 0.0 and css[5] == 0.0
        pop = np.nan_to_num(b[flags].astype(np.float64))
        for j in range(4):
            exact = mr.exact_css_about(pop[:, j], mean[j])
            err = abs(Fraction(float(css[j])) - exact) / exact
            print('css column %d (%s, %s): off by %.2f x 2^-53 relative, bound %d' % (j, np.dtype(dtype).name, order, float(err / Fraction(mr.U)), n_v + 4))
            assert err <= (n_v + 4) * Fraction(mr.U), (j, float(err))
        again = attr.column_moments()
        assert np.array_equal(bits(again[0]), bits(mean)) and np.array_equal(bits(again[1]), bits(css))
    finally:
        attr.close()


# ------------------------------------------------------------------------------------------------------- T2, T3, T4 ----

@pytest.fixture(scope='module')
def designed_run(be, ctx):
    """The designed case through safe_moments_test once ('both', 0.05, with z) with what the checks need beside it."""
    case = mr.designed()[0]
    nbr, attr = handles(be, ctx, case)
    try:
        out = run_moments(be, ctx, nbr, attr)
        mean, css = attr.column_moments()
        score = observed_scores(be, ctx, nbr, attr)
    finally:
        attr.close()
        nbr.close()
    return case, out, mean, css, score


def test_designed_cells(designed_run, k_ref):
    case, out, mean, css, score = designed_run
    assert np.array_equal(bits(out['ns']), bits(score)) and np.array_equal(out['ns'], case.x)
    n_deg, n_cells = check_cells(out, case.k, case.n_v, mean, css, k_ref, 'designed')
    z, kinds = mr.designed_z()
    assert n_deg == sum(kinds.values()) - kinds['n_v < 2'] and n_cells == len(case.cells())      # no designed cell is skipped
    check_outputs(out, 'both', 0.05, 'designed')
    assert np.isinf(out['nes']).any() and (out['nes'] < 0).any() and (out['nes_binary'] == 1).any()


@pytest.mark.parametrize('thr', [0.05, 1e-9])
@pytest.mark.parametrize('sign', mr.SIGNS)
def test_designed_signs_and_thresholds(be, ctx, designed_run, sign, thr):
    case, first, _, _, _ = designed_run
    nbr, attr = handles(be, ctx, case)
    try:
        out = run_moments(be, ctx, nbr, attr, sign, thr)
        bare = run_moments(be, ctx, nbr, attr, sign, thr, want_z=False)
    finally:
        attr.close()
        nbr.close()
    for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'z'):
        assert np.array_equal(bits(out[name]), bits(first[name])), name
    check_outputs(out, sign, thr, 'designed %s %g' % (sign, thr))
    for name in OUTPUTS:                                        # z_dev = NULL: the same other outputs, bit for bit
        assert np.array_equal(bits(bare[name]), bits(out[name])), name
    assert 0 < out['nes_binary'].sum() < out['nes_binary'].size


def test_a_population_of_one_row(be, ctx, k_ref):
    case = mr.designed()[1]
    nbr, attr = handles(be, ctx, case)
    try:
        out = run_moments(be, ctx, nbr, attr)
        mean, css = attr.column_moments()
    finally:
        attr.close()
        nbr.close()
    n_deg, n_cells = check_cells(out, case.k, case.n_v, mean, css, k_ref, 'n_v = 1')
    assert n_deg == n_cells == len(case.cells())
    assert np.array_equal(out['nes_binary'], np.zeros_like(out['nes_binary']))
    check_outputs(out, 'both', 0.05, 'n_v = 1')


# rows against the emit tile (1, 2, 15, 16, 17, 33, 2048), columns against the lanes and the column chunk (1, 63, 64, 65, 1023,
# 1024, 1025); every storage form and order; sub-ranges that start past column 0
SWEEP = [(1, 1, np.float64, 'C', None), (2, 63, np.float32, 'F', None), (ROW_TILE - 1, LANES, np.float64, 'F', (1, 64)),
         (ROW_TILE, LANES + 1, np.uint8, 'C', None), (ROW_TILE + 1, COL_CHUNK - 1, np.float32, 'C', (7, 1023)),
         (2 * ROW_TILE + 1, COL_CHUNK, np.float64, 'C', None), (ROW_CHUNK, COL_CHUNK + 1, np.uint8, 'F', None),
         (2 * ROW_TILE + 1, COL_CHUNK + 1, 'sparse', 'F', (0, 1025)), (ROW_CHUNK + 1, LANES + 1, np.float32, 'F', (64, 65))]


@pytest.mark.parametrize('n,m,dtype,order,cols', SWEEP, ids=lambda v: getattr(v, '__name__', str(v)))
def test_shapes_layouts_and_column_ranges(be, ctx, k_ref, n, m, dtype, order, cols):
    integers = dtype == np.uint8
    case = mr.periodic_case(n, m, 100 * n + m, integers=integers, missing=not integers)
    col0, col1 = cols or (0, m)
    nbr = be.Neighborhoods.from_dense(ctx, case.a)
    if dtype == 'sparse':
        import scipy.sparse as sp
        stored = case.b.copy()
        stored[~case.flags] = 0                                 # rows without a value come as missing_rows, NaN cells stay stored
        attr = be.Attributes.from_sparse(ctx, sp.csc_array(stored), missing_rows=(~case.flags).astype(np.uint8))
        values = case.b
    else:
        host = np.nan_to_num(case.b).astype(np.uint8) if integers else case.b.astype(dtype)
        attr = be.Attributes.from_host(ctx, np.asarray(host, order=order))
        values = host.astype(np.float64)
    try:
        out = run_moments(be, ctx, nbr, attr, col0=col0, col1=col1)
        mean, css = attr.column_moments(col0, col1)
        score = observed_scores(be, ctx, nbr, attr, col0, col1)
        whole = attr.column_moments()
        assert attr.stats()['n_rows_with_value'] == case.n_v
    finally:
        attr.close()
        nbr.close()
    what = 'shape %d x %d %s %s [%d, %d)' % (n, m, getattr(dtype, '__name__', dtype), order, col0, col1)
    assert np.array_equal(bits(mean), bits(whole[0][col0:col1])) and np.array_equal(bits(css), bits(whole[1][col0:col1])), what
    assert np.array_equal(bits(out['ns']), bits(score)), what
    np.testing.assert_allclose(out['ns'], (case.a @ np.nan_to_num(values))[:, col0:col1], rtol=1e-12, atol=1e-9, err_msg=what)
    # every cell equals its representative among the 5 distinct neighborhoods x 7 distinct columns, bit for bit ...
    rows, columns = np.arange(n) % 5, (np.arange(col0, col1) % 7)
    first_col = {c: j for j, c in reversed(list(enumerate(columns)))}
    rep_cols = np.array([first_col[c] for c in columns])
    for name in ('ns', 'z', 'pvalues_pos', 'pvalues_neg', 'nes', 'nes_binary'):
        assert np.array_equal(bits(out[name]), bits(out[name][rows][:, rep_cols])), '%s: %s is not periodic' % (what, name)
    # ... and the representatives are checked exactly
    keep_r, keep_c = np.arange(min(n, 5)), np.array(sorted(set(rep_cols.tolist())))
    sub = {name: out[name][np.ix_(keep_r, keep_c)] for name in ('ns', 'z', 'pvalues_pos', 'pvalues_neg')}
    check_cells(sub, case.k[keep_r], case.n_v, mean[keep_c], css[keep_c], k_ref, what)
    check_outputs(out, 'both', 0.05, what)


# ----------------------------------------------------------------------------------------------------------------- T5 ----

N, RADIUS, THR = 300, 0.2, 0.05


def api_matrix(kind):
    """(load_attributes kwargs, the dense f64 equivalent): the 40 golden annotations, three small-integer columns, a constant."""
    import os
    import scipy.sparse as sp
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'domains.npz'))
    r = np.arange(N)
    b = np.concatenate([g['attributes'], ((r * 7) % 5)[:, None], ((r * 3) % 11)[:, None], (r % 2 * 4)[:, None], np.full((N, 1), 2.0)], axis=1).astype(np.float64)
    missing = np.zeros(N, dtype=bool)
    if kind != 'uint8':
        missing[np.random.default_rng(78).choice(N, 8, replace=False)] = True
        b[missing] = np.nan
    if kind == 'uint8':
        return {'attribute_file': b.astype(np.uint8)}, b
    if kind == 'sparse':
        return {'attribute_file': sp.csc_array(np.nan_to_num(b)), 'missing_rows': missing.astype(np.uint8)}, b
    return {'attribute_file': b.astype(np.float32 if kind == 'f32' else np.float64)}, b


def new_safe(amd, load, sign='both'):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'domains.npz'))
    xy, eu, ev = g['xy'], g['edge_u'], g['edge_v']
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1)))
    sf.attribute_sign = sign
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=RADIUS)
    sf.load_attributes(**load)
    return sf


def resident(sf, names=('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')):
    from safepy_amd.safe import _DeviceResult
    return [isinstance(sf.__dict__.get('_r_' + name), _DeviceResult) for name in names]


@pytest.mark.parametrize('kind', ['f64', 'f32', 'uint8', 'sparse'])
def test_t5_compute_pvalues_analytic(amd, k_ref, kind):
    """Against the restatement on the host's values: exact z (Fractions), mpmath tails.  The device's z may be off by the T2
    bound, by the rounded mean (2^-53 |k mu| / sd) and by the css bound ((n_v + 4) 2^-53 / 2 relative); a shift dz moves the
    small side by at most (|z| + 1) dz relative (the normal hazard rate is below |z| + 1), on top of the T3 bound."""
    load, b = api_matrix(kind)
    sf = new_safe(amd, load)
    sf.compute_pvalues(how='analytic', num_permutations=10, random_seed=3)          # (both ignored)
    assert sf.enrichment_type == 'analytic' and sf._ctx().last_kernel()[0] == 'k_moments_emit'
    assert all(resident(sf)), 'the results were read back before anyone asked'
    a = np.array(sf.neighborhoods, dtype=np.float64)
    flags, n_v, mu, q = mr.exact_moments(b)
    k = (a @ flags.astype(np.float64)).astype(np.int64)
    x = a @ np.nan_to_num(b)
    ns, pp, pn, nes = (np.array(getattr(sf, name)) for name in ('ns', 'pvalues_pos', 'pvalues_neg', 'nes'))
    assert np.array_equal(ns, x)
    small, checked = np.minimum(pp, pn), 0
    for j in range(b.shape[1]):
        for kk, xx in set(zip(k.tolist(), x[:, j].tolist())):
            cells = (k == kk) & (x[:, j] == xx)
            z, sd, kmu = mr.exact_z(Fraction(xx), kk, n_v, mu[j], q[j])
            if z is None:
                assert (pp[cells, j] == 1).all() and (pn[cells, j] == 1).all() and (nes[cells, j] == 0).all()
                continue
            az = abs(z)
            dz = mr.U * ((C_OPS + (n_v + 4) / 2) * az + 3 * abs(kmu) / sd)
            want = mr.small_side(z)
            got = small[cells, j]
            assert (got == got[0]).all()
            if az <= mr.Z_EDGE - 0.1:
                err = abs(mr.MP.mpf(float(got[0])) - want) / want
                assert err <= (az + 1) * dz + 2 * k_ref * (1 + az ** 2) * mr.U, (kind, j, kk, xx, float(err))
                side_pos = pp[cells, j][0] <= pn[cells, j][0]
                assert side_pos == (z >= 0) or az < 1e-9
                checked += 1
    assert checked > 1000
    upper = pp <= pn
    assert np.array_equal(bits(np.where(upper, pn, pp))[small < 1], bits(1.0 - small)[small < 1])
    # on the parent this call ran the permutation test: every p-value a multiple of 1 / num_permutations
    assert not np.array_equal(pp * 1000, np.round(pp * 1000)) and (pp[pp > 0] < 1e-4).any()
    check_outputs({'pvalues_pos': pp, 'pvalues_neg': pn, 'nes': nes, 'nes_binary': np.array(sf.nes_binary),
                   'num_enriched': np.array(sf.attributes['num_neighborhoods_enriched'].values, dtype=np.float64)}, 'both', THR, kind)


def test_t5_multiple_testing_downstream_and_the_other_routes(amd):
    from oracle import safe_oracle as orc
    load, b = api_matrix('f64')
    sf = new_safe(amd, load, 'highest')
    sf.compute_pvalues(how='analytic')
    plain = {name: np.array(getattr(sf, name)) for name in ('ns', 'pvalues_pos', 'pvalues_neg')}
    sf.compute_pvalues(how='analytic', multiple_testing=True)
    assert all(resident(sf))
    sf.define_top_attributes()                                  # runs on the resident nes_binary
    assert resident(sf, ('nes_binary',)) == [True] and 'top' in sf.attributes
    pp, pn, nes = (np.array(getattr(sf, name)) for name in ('pvalues_pos', 'pvalues_neg', 'nes'))
    assert np.array_equal(np.array(sf.ns), plain['ns'])
    assert np.array_equal(pp, orc.fdr_rows(plain['pvalues_pos'])) and np.array_equal(pn, orc.fdr_rows(plain['pvalues_neg']))
    check_outputs({'pvalues_pos': pp, 'pvalues_neg': pn, 'nes': nes, 'nes_binary': np.array(sf.nes_binary),
                   'num_enriched': np.array(sf.attributes['num_neighborhoods_enriched'].values, dtype=np.float64)}, 'highest', THR, 'fdr')
    # the other routes on the same instance afterwards
    sf.random_seed = 1
    sf.compute_pvalues(how='randomization', multiple_testing=False, num_permutations=50)
    a = np.array(sf.neighborhoods)
    want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', num_permutations=50, random_seed=1, attribute_sign='highest')
    for key in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):
        assert np.array_equal(np.array(getattr(sf, key)), want[key]), key
    sf.load_attributes(attribute_file=(np.nan_to_num(b[:, :40])).copy())
    sf.compute_pvalues(how='hypergeometric')
    want = orc.compute_pvalues(a, np.nan_to_num(b[:, :40]), enrichment_type='hypergeometric')
    assert np.allclose(np.array(sf.pvalues_pos), want['pvalues_pos'], rtol=1e-6, atol=1e-300)
    assert np.array_equal(np.array(sf.nes_binary), want['nes_binary'])


def test_t5_z_scores_are_refused_with_nothing_launched(amd):
    from safepy_amd import backend as be
    sf = new_safe(amd, api_matrix('f64')[0])
    sf.compute_pvalues(how='analytic')
    kernel, live, before = sf._ctx().last_kernel(), be.device_live_alloc_count(), sf.__dict__.get('_r_nes')
    with pytest.raises(ValueError, match="'sum' only"):
        sf.compute_pvalues(how='analytic', neighborhood_score_type='z-score')
    assert sf._ctx().last_kernel() == kernel and be.device_live_alloc_count() == live and sf.__dict__.get('_r_nes') is before


# ----------------------------------------------------------------------------------------------------------------- T6 ----

def test_t6_refusals_leave_no_allocation(be, ctx):
    case = mr.periodic_case(20, 10, 9)
    nbr, attr = handles(be, ctx, case)
    other = be.Attributes.from_host(ctx, np.zeros((21, 10)))
    lib, E = be._lib.lib, be._lib
    bufs = [ctx.alloc_f64(20, 10) for _ in range(5)] + [ctx.alloc_f64(10)]
    ptrs = [buf.ptr for buf in bufs]
    marker = np.full((20, 10), -3.0)
    mean, css = np.empty(10), np.empty(10)

    def code(fn):
        with pytest.raises(be._lib.SafeHipError) as err:
            fn()
        return err.value.code

    def raw(sign, thr=0.05):
        be.check(lib.safe_moments_test(ctx.handle, nbr.handle, attr.handle, sign, thr, 0, 10, *[C.c_void_p(p) for p in ptrs], None))

    def raw_moments(handle, col0, col1, mean_ptr, css_ptr):
        be.check(lib.safe_attr_column_moments(handle, col0, col1, mean_ptr, css_ptr))

    try:
        run_moments(be, ctx, nbr, attr)                         # the scratch slots have their sizes
        for buf in bufs[:5]:
            buf.upload(marker)
        live = be.device_live_alloc_count()
        for i in range(6):                                      # every output but z is needed
            assert code(lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, ptrs[:i] + [None] + ptrs[i + 1:])) == E.E_INVALID
        assert code(lambda: be.moments_test(ctx, nbr, other, 'both', 0.05, ptrs)) == E.E_INVALID             # 20 against 21 rows
        assert code(lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, ptrs, 0, 11)) == E.E_INVALID
        assert code(lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, ptrs, 5, 5)) == E.E_INVALID
        assert code(lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, ptrs, -1, 5)) == E.E_INVALID
        for thr in (0.0, 1.0, -0.5, float('nan')):
            assert code(lambda: raw(2, thr)) == E.E_INVALID
        assert code(lambda: raw(3)) == E.E_INVALID and code(lambda: raw(-1)) == E.E_INVALID
        ptr = lambda v: v.ctypes.data_as(C.c_void_p)            # noqa: E731
        assert code(lambda: raw_moments(None, 0, 10, ptr(mean), ptr(css))) == E.E_INVALID
        assert code(lambda: raw_moments(attr.handle, 0, 10, None, ptr(css))) == E.E_INVALID
        assert code(lambda: raw_moments(attr.handle, 0, 10, ptr(mean), None)) == E.E_INVALID
        assert code(lambda: raw_moments(attr.handle, 0, 11, ptr(mean), ptr(css))) == E.E_INVALID
        assert code(lambda: raw_moments(attr.handle, 4, 4, ptr(mean), ptr(css))) == E.E_INVALID
        assert be.device_live_alloc_count() == live
        for buf in bufs[:5]:
            assert np.array_equal(buf.download((20, 10)), marker)                                  # nothing was written
        run_moments(be, ctx, nbr, attr)                         # the context still works
    finally:
        for buf in bufs:
            buf.free()
        for h in (other, attr, nbr):
            h.close()


def test_t6_on_a_busy_caller_stream(be, ctx):
    """safe_moments_test on a caller's stream that is still busy producing its input, outputs poisoned: the same bits as a
    quiet run (the harness of tests/test_gpu_stream_order.py)."""
    import torch
    import test_gpu_stream_order as so
    lab = so.Lab(be, ctx, torch)
    nbr = None
    try:
        case = mr.periodic_case(301, 70, 4)
        n, m = case.b.shape
        nbr = be.Neighborhoods.from_dense(ctx, case.a)
        bor = so.Borrowed(lab, case.b)
        attr = bor.handle(lab)
        outs = [torch.empty((n, m), dtype=torch.float64, device='cuda') for _ in range(5)] + [torch.empty((m,), dtype=torch.float64, device='cuda'),
                                                                                                 torch.empty((n, m), dtype=torch.float64, device='cuda')]
        fn = lambda: be.moments_test(ctx, nbr, attr, 'both', 0.05, [o.data_ptr() for o in outs[:6]], z_ptr=outs[6].data_ptr())   # noqa: E731

        def check(got):
            from scipy.special import ndtr
            np.testing.assert_allclose(got[0], case.a @ np.nan_to_num(case.b), rtol=1e-12, atol=1e-9)
            live = got[2] < 1
            np.testing.assert_allclose(got[2][live], ndtr(-got[6][live]), rtol=1e-9, atol=1e-300)
            assert np.array_equal(got[5], got[4].sum(axis=0))
        call = so.Call(['safe_moments_test'], [(bor.tensor, bor.staging)], outs, fn, check, done=attr.close)
        try:
            quiet, t_call_ms = so.run_quiet(lab, call)
            call.check(quiet)
            busy, _ = so.run_busy(lab, call, t_call_ms)
        finally:
            call.done()
        for i, (q, v) in enumerate(zip(quiet, busy)):
            assert np.array_equal(so.bits(v), so.bits(q)), 'output %d of the busy run differs from the quiet run' % i
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        if nbr is not None:
            nbr.close()


def test_t6_no_live_block_left_behind(be, ctx):
    case = mr.periodic_case(ROW_CHUNK, COL_CHUNK + 1, 8)
    nbr, attr = handles(be, ctx, case, np.float32, 'F')
    n, m = case.b.shape
    bufs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
    try:
        be.moments_test(ctx, nbr, attr, 'both', 0.05, [b.ptr for b in bufs])      # the scratch slots grow to their sizes
        attr.column_moments()
        before = be.device_live_alloc_count()
        for sign in mr.SIGNS:
            be.moments_test(ctx, nbr, attr, sign, 0.05, [b.ptr for b in bufs])
            attr.column_moments(5, 900)
        assert be.device_live_alloc_count() == before
    finally:
        for b in bufs:
            b.free()
        attr.close()
        nbr.close()


def test_zz_worst_errors_seen():
    print('worst |dz| as a share of its bound: %.3f' % WORST_Z[0])
    for bucket in sorted(WORST_P):
        print('|z| >= %-5g worst p error %.3f (1 + z^2) 2^-53' % (bucket, WORST_P[bucket]))
    assert WORST_P and WORST_Z[0] <= 1.0
