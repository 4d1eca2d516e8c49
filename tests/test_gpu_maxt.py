"""The two entry points of the max-statistic adjustment (include/safe_hip.h: safe_permtest_extremes, safe_counts_from_extremes;
safepy_amd/csrc/maxt.hip) against tests/maxt_ref.py: z, the live flags, tmax and tmin bit for bit, the counts exactly.  Needs an
MI355X.

Constants of maxt.hip the shapes are chosen around (both sides of each):
  MX_BN = 16     columns of a tile; tiles are dealt to 8 queues (blockIdx % 8)
  MX_RB = 16     rows of a chunk; a workgroup walks every n_groups-th chunk
  64 / 256       permutations of a wave / of a workgroup of k_maxt_extremes (a wave past the table's end idles at the barriers)
  CT_PC = 32     permutations k_maxt_counts stages per pass: P <= 32 is one pass, every larger P repeats it (the one form for any
                 P: the count stage is N M P compares, 1 / (members per neighborhood) of the extremes kernel's gathers)
  CT_RT = 16, 64 rows a lane / a block of k_maxt_counts holds; 64 columns per block

mu_j and Q_j come from Attributes.column_moments (safe_attr_column_moments), as the contract says; everything else is restated."""
import numpy as np
import pytest

import maxt_ref as mx
import weights_ref as wr

pytestmark = pytest.mark.gpu

POISON = -12345.678
POISON_BYTE = 0xA5
GUARD = 64


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    assert np.array_equal(bits(got), bits(want)), what


def membership(n, seed, dense_row=False):
    rng = np.random.default_rng(seed)
    a = rng.uniform(size=(n, n)) < min(1.0, 12.0 / n)
    a[np.arange(n), np.arange(n)] = True
    if n >= 3:
        a[1] = False                                            # an empty row
    if dense_row:
        a[0] = True                                             # one row of n members
    return a.astype(np.int64)


def attributes(n, m, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 4, size=(n, m)).astype(np.uint8)
    b = np.round(rng.normal(size=(n, m)) * 3, 3)
    if n >= 4:
        b[rng.uniform(size=b.shape) < 0.05] = np.nan           # NaN cells
        b[rng.choice(n, max(1, n // 8), replace=False)] = np.nan   # members without a value
    return b.astype(dtype)


def make_perms(be, ctx, how, n, flags, count, seed):
    if how == 'seeded':
        return be.Permutations(ctx, n, flags, count, seed)
    if how == 'device':
        return be.Permutations(ctx, n, flags, count, None, device_key=0xC0FFEE + seed)
    if how == 'stratified':
        return be.Permutations.stratified(ctx, n, flags, (np.arange(n) % 3).astype(np.int32), count, 0xBEEF + seed)
    return be.Permutations.from_table(ctx, mx.random_tables(n, flags, count, np.random.default_rng(seed)))


class Poisoned:
    """Device buffers filled with a pattern, with a guard band behind the part a call may write."""

    def __init__(self, ctx, shapes):
        self.shapes = shapes
        self.bufs = {}
        for name, (shape, dtype) in shapes.items():
            size = int(np.prod(shape)) + GUARD
            buf = ctx.alloc(size * np.dtype(dtype).itemsize)
            buf.upload(np.full(size, POISON_BYTE if dtype == np.uint8 else POISON, dtype=dtype))
            self.bufs[name] = buf

    def ptr(self, name):
        return self.bufs[name].ptr

    def read(self, name, written=True):
        shape, dtype = self.shapes[name]
        size = int(np.prod(shape))
        flat = self.bufs[name].download((size + GUARD,), dtype=dtype)
        pattern = POISON_BYTE if dtype == np.uint8 else POISON
        assert (flat[size:] == pattern).all(), '%s: the call wrote past the end of its output' % name
        if not written:
            assert (flat == pattern).all(), '%s: a refused call wrote into its output' % name
        return flat[:size].reshape(shape).copy()

    def free(self):
        for b in self.bufs.values():
            b.free()


def run_extremes(be, ctx, nbr, attr, perms, col0=0, col1=None):
    n, m, P = attr.n, (attr.m if col1 is None else col1) - col0, perms.count
    out = Poisoned(ctx, {'z': ((n, m), np.float64), 'live': ((n, m), np.uint8), 'tmax': ((P, m), np.float64), 'tmin': ((P, m), np.float64)})
    try:
        be.permtest_extremes(ctx, nbr, attr, perms, out.ptr('z'), out.ptr('live'), out.ptr('tmax'), out.ptr('tmin'), col0, col1)
        assert ctx.last_kernel()[0] == 'k_maxt_extremes'
        return {name: out.read(name) for name in out.shapes}
    finally:
        out.free()


def run_counts(be, ctx, ext, scope):
    n, m = ext['z'].shape
    P = len(ext['tmax'])
    inputs = {name: ctx.alloc(ext[name].nbytes) for name in ('z', 'live', 'tmax', 'tmin')}
    out = Poisoned(ctx, {'neg': ((n, m), np.float64), 'pos': ((n, m), np.float64), 'least_neg': ((m,), np.float64),
                         'least_pos': ((m,), np.float64)})
    try:
        for name, buf in inputs.items():
            buf.upload(ext[name])
        be.counts_from_extremes(ctx, n, m, P, scope, *[inputs[k].ptr for k in ('z', 'live', 'tmax', 'tmin')], out.ptr('neg'),
                                out.ptr('pos'), out.ptr('least_neg'), out.ptr('least_pos'))
        assert ctx.last_kernel()[0] == 'k_maxt_counts'
        return [out.read(name) for name in ('neg', 'pos', 'least_neg', 'least_pos')]
    finally:
        out.free()
        for buf in inputs.values():
            buf.free()


def reference(a, b64, w, attr, tables, col0=0, col1=None):
    """The restatement on the device's own column moments and row flags."""
    col1 = b64.shape[1] if col1 is None else col1
    indptr, indices = wr.csr_of(a)
    flags = attr.row_flags() != 0
    mu, q = attr.column_moments(col0, col1)
    loc, scale = mx.row_factors(indptr, indices, flags, int(flags.sum()), w)
    return mx.extremes(indptr, indices, w, b64[:, col0:col1], tables, loc, scale, mu, q)


def check_all(be, ctx, a, host, w, how, count, seed, sub=None, what=''):
    """Extremes and both scopes' counts of one input against the restatement; `host` is what Attributes.from_host takes."""
    import scipy.sparse as sp
    b64 = np.asarray(host.toarray() if sp.issparse(host) else host, dtype=np.float64)
    n = len(a)
    nbr = be.Neighborhoods.from_dense(ctx, np.asarray(a, dtype=np.int64))
    attr = be.Attributes.from_host(ctx, host)
    perms = make_perms(be, ctx, how, n, (attr.row_flags() != 0).astype(np.uint8), count, seed)
    try:
        if w is not None:
            nbr.set_weights(w)
        tables = perms.read().astype(np.int64)
        for col0, col1 in [(0, None)] + ([sub] if sub else []):
            got = run_extremes(be, ctx, nbr, attr, perms, col0, col1)
            z, live, tmax, tmin, _ = reference(a, b64, w, attr, tables, col0, col1)
            same_bits(got['z'], z, what + ' z')
            assert np.array_equal(got['live'], live.astype(np.uint8)), what + ' live'
            same_bits(got['tmax'], tmax, what + ' tmax')
            same_bits(got['tmin'], tmin, what + ' tmin')
            for scope, code in (('neighborhoods', mx.COLUMN), ('all', mx.MATRIX)):
                have = run_counts(be, ctx, got, scope)
                want = mx.counts(z, live, tmax, tmin, code)
                for p, q, name in zip(have, want, ('counts_neg', 'counts_pos', 'min_counts_neg', 'min_counts_pos')):
                    assert np.array_equal(p, q), '%s %s %s' % (what, scope, name)
        return got
    finally:
        perms.close()
        attr.close()
        nbr.close()


def custom_weights(a, seed):
    indptr, indices = wr.csr_of(a)
    w = 1.0 - np.random.default_rng(seed).uniform(size=len(indices))
    w[::4] = 0.0                                                # zero weights stay members
    return w


# n: one chunk (1, 2), four chunks and both sides of it (63, 64, 65), 17 and 129 chunks; m: below a tile, 15 / 16 / 17, three
# tiles (33) with a sub-range that starts inside the first one; P: one pass of the count stage (1, 3), both sides of a wave of
# the extremes kernel and two passes (63, 64, 65), three waves (130), five workgroups of permutations (1025, on a small n)
CASES = [('table', 1, 1, 1, False, np.float64, 'C', None),
         ('seeded', 2, 15, 3, False, np.float32, 'F', None),
         ('device', 63, 16, 63, True, np.float64, 'C', None),
         ('stratified', 64, 17, 64, True, np.float64, 'F', (5, 16)),
         ('table', 65, 33, 65, False, np.uint8, 'C', (5, 30)),
         ('seeded', 257, 9, 130, True, np.float32, 'C', (3, 8)),
         ('device', 2049, 5, 3, False, np.float64, 'C', None),
         ('stratified', 33, 3, 1025, True, np.float64, 'C', None)]


@pytest.mark.parametrize('how,n,m,count,weighted,dtype,order,sub', CASES)
def test_extremes_and_counts(be, ctx, how, n, m, count, weighted, dtype, order, sub):
    a = membership(n, n * 7 + m, dense_row=n == 2049)            # (2049: one row of 2049 members)
    b = np.asarray(attributes(n, m, n + count, dtype), order=order)
    w = custom_weights(a, n + m) if weighted else None
    check_all(be, ctx, a, b, w, how, count, seed=n + m, sub=sub, what='%s n=%d m=%d P=%d' % (how, n, m, count))


def test_sparse_input_and_dense_row_with_weights(be, ctx):
    import scipy.sparse as sp
    rng = np.random.default_rng(8)
    n, m = 300, 20
    dense = np.where(rng.uniform(size=(n, m)) < 0.2, np.round(rng.normal(size=(n, m)), 2), 0.0)
    a = membership(n, 3, dense_row=True)
    check_all(be, ctx, a, sp.csc_matrix(dense), None, 'device', 10, seed=1, what='csc flat')
    check_all(be, ctx, a, sp.csc_matrix(dense), custom_weights(a, 2), 'table', 10, seed=2, what='csc weighted')


def test_triangular_weights_from_the_layout(be, ctx):
    rng = np.random.default_rng(9)
    n, m, count = 130, 7, 20
    xy = rng.uniform(size=(n, 2))
    b = attributes(n, m, 4)
    nbr = be.Neighborhoods.euclidean(ctx, xy, 0.2)
    attr = be.Attributes.from_host(ctx, b)
    perms = make_perms(be, ctx, 'seeded', n, (attr.row_flags() != 0).astype(np.uint8), count, 5)
    try:
        nbr.set_weights_from_xy(xy, 'triangular', 0.2)
        w = nbr.weights()
        assert (w == 0).any() or (w < 0.05).any()
        a = nbr.to_dense()
        got = run_extremes(be, ctx, nbr, attr, perms)
        z, live, tmax, tmin, _ = reference(a, b, w, attr, perms.read().astype(np.int64))
        same_bits(got['z'], z, 'z')
        same_bits(got['tmax'], tmax, 'tmax')
        same_bits(got['tmin'], tmin, 'tmin')
    finally:
        perms.close()
        attr.close()
        nbr.close()


def test_degenerate_cells_and_columns(be, ctx):
    """k_i = 0 (an empty row, and a row whose only member holds no value), k_i = n_v, a constant column (every cell degenerate:
    -inf / +inf extremes, count P), the whole population at one weight."""
    rng = np.random.default_rng(3)
    n, m, count = 70, 18, 40
    a = membership(n, 6)
    b = np.round(rng.normal(size=(n, m)), 2)
    b[60:] = np.nan                                             # n_v = 60
    a[0] = 0
    a[0, 65] = 1                                                # k_0 = 0 with a member
    a[2, :] = 1                                                 # k_2 = n_v
    b[:60, 16] = 7.0                                            # a constant column in the second tile
    b[5, 3] = np.nan
    for w in (None, custom_weights(a, 1)):
        if w is not None:
            indptr, _ = wr.csr_of(a)
            w[indptr[2]:indptr[3]] = 0.375                      # the whole population at one weight
        got = check_all(be, ctx, a, b, w, 'device', count, seed=7, what='degenerate')
        assert not got['live'][[0, 1, 2]].any() and not got['live'][:, 16].any() and got['live'][3:, :16].all()
        assert np.isneginf(got['tmax'][:, 16]).all() and np.isposinf(got['tmin'][:, 16]).all()
        assert (got['z'][got['live'] == 0] == 0).all()
        neg, pos, least_neg, least_pos = run_counts(be, ctx, got, 'all')
        assert (neg[got['live'] == 0] == count).all() and (pos[got['live'] == 0] == count).all()
        assert least_neg[16] == count and least_pos[16] == count


def test_ties_pin_the_comparisons(be, ctx):
    """Equal-sized neighborhoods and 0/1 data: equal sums are equal z bits, and they are frequent -- a count with > for >= (or <
    for <=) would differ in most cells."""
    a, b = mx.tied_case(96, 6, 12)
    got = check_all(be, ctx, a, b, None, 'seeded', 64, seed=3, what='ties')
    assert (got['tmax'][:, :, None] == got['z'].T[None, :, :]).any()         # observed statistics that tie with an extreme
    assert (got['tmin'][:, :, None] == got['z'].T[None, :, :]).any()
    assert len(np.unique(got['z'])) <= 6 * 6                                 # at most six sums per column


def test_order_sensitive_input(be, ctx):
    a, b, indptr, indices, w = wr.order_sensitive(300, 5, seed=31)
    check_all(be, ctx, a, b, w, 'seeded', 10, seed=4, what='order-sensitive weighted')
    check_all(be, ctx, a, b, None, 'seeded', 10, seed=4, what='order-sensitive flat')
    # the restatement with the members added in descending order differs: the check above can see the order
    x_up = wr.score(indptr, indices, w, b)
    x_down = wr.score(indptr, indices, w, b, descending=True)
    assert (bits(x_up) != bits(x_down)).any()


def test_z_is_the_analytic_tests_and_unit_weights_are_flat(be, ctx):
    """z_dev has the bits of the z of safe_moments_test (flat) and safe_moments_test_weighted (weights); a handle with unit
    weights gives the bytes of the flat handle; identical calls give identical bytes; device memory is steady."""
    n, m, count = 257, 33, 20
    a = membership(n, 21)
    b = attributes(n, m, 22)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    attr = be.Attributes.from_host(ctx, b)
    perms = make_perms(be, ctx, 'device', n, (attr.row_flags() != 0).astype(np.uint8), count, 2)
    outs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m), ctx.alloc_f64(n, m)]
    try:
        flat = run_extremes(be, ctx, nbr, attr, perms)
        be.moments_test(ctx, nbr, attr, 'both', 0.05, [x.ptr for x in outs[:6]], z_ptr=outs[6].ptr)
        same_bits(flat['z'], outs[6].download((n, m)), 'z of safe_moments_test')
        nbr.set_weights(np.ones(nbr.nnz))
        unit = run_extremes(be, ctx, nbr, attr, perms)
        for name in flat:
            assert np.array_equal(flat[name].view(np.uint8), unit[name].view(np.uint8)), 'unit weights: ' + name
        nbr.set_weights(custom_weights(a, 5))
        first = run_extremes(be, ctx, nbr, attr, perms)
        be.moments_test_weighted(ctx, nbr, attr, 'both', 0.05, [x.ptr for x in outs[:6]], z_ptr=outs[6].ptr)
        same_bits(first['z'], outs[6].download((n, m)), 'z of safe_moments_test_weighted')
        live = be.device_live_alloc_count()
        for _ in range(3):
            again = run_extremes(be, ctx, nbr, attr, perms)
            for name in first:
                assert np.array_equal(first[name].view(np.uint8), again[name].view(np.uint8)), 'identical calls: ' + name
            for scope in ('neighborhoods', 'all'):
                run_counts(be, ctx, again, scope)
        assert be.device_live_alloc_count() == live
        # without z and without flags: the extremes alone
        bare = Poisoned(ctx, {'tmax': ((count, m), np.float64), 'tmin': ((count, m), np.float64)})
        try:
            be.permtest_extremes(ctx, nbr, attr, perms, None, None, bare.ptr('tmax'), bare.ptr('tmin'))
            same_bits(bare.read('tmax'), first['tmax'], 'tmax without z')
            same_bits(bare.read('tmin'), first['tmin'], 'tmin without z')
        finally:
            bare.free()
    finally:
        for x in outs:
            x.free()
        perms.close()
        attr.close()
        nbr.close()


def test_whole_matrix_family_is_the_fold_of_the_columns(be, ctx):
    n, m, count = 65, 130, 33
    a = membership(n, 2)
    b = attributes(n, m, 3)
    got = check_all(be, ctx, a, b, None, 'table', count, seed=9, what='fold')
    col = run_counts(be, ctx, got, 'neighborhoods')
    folded = dict(got)
    folded['tmax'] = np.ascontiguousarray(np.broadcast_to(got['tmax'].max(axis=1)[:, None], got['tmax'].shape))
    folded['tmin'] = np.ascontiguousarray(np.broadcast_to(got['tmin'].min(axis=1)[:, None], got['tmin'].shape))
    want = run_counts(be, ctx, folded, 'neighborhoods')
    have = run_counts(be, ctx, got, 'all')
    for p, q in zip(have, want):
        assert np.array_equal(p, q)
    assert (have[1] >= col[1]).all() and (have[0] >= col[0]).all()


def test_refusals_write_nothing(amd, be, ctx):
    n, m, count = 65, 9, 10
    a = membership(n, 1)
    b = attributes(n, m, 2)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    attr = be.Attributes.from_host(ctx, b)
    small = be.Attributes.from_host(ctx, b[:64])
    small_nbr = be.Neighborhoods.from_dense(ctx, a[:64, :64])
    perms = make_perms(be, ctx, 'device', n, (attr.row_flags() != 0).astype(np.uint8), count, 1)
    out = Poisoned(ctx, {'z': ((n, m), np.float64), 'live': ((n, m), np.uint8), 'tmax': ((count, m), np.float64),
                         'tmin': ((count, m), np.float64), 'neg': ((n, m), np.float64), 'pos': ((n, m), np.float64),
                         'least_neg': ((m,), np.float64), 'least_pos': ((m,), np.float64)})
    z, live, tmax, tmin = (out.ptr(k) for k in ('z', 'live', 'tmax', 'tmin'))
    tail = (out.ptr('neg'), out.ptr('pos'), out.ptr('least_neg'), out.ptr('least_pos'))
    try:
        refused = [lambda: be.permtest_extremes(ctx, nbr, attr, perms, z, live, None, tmin),
                   lambda: be.permtest_extremes(ctx, nbr, attr, perms, z, live, tmax, None),
                   lambda: be.permtest_extremes(ctx, nbr, attr, perms, z, live, tmax, tmin, 3, 3),
                   lambda: be.permtest_extremes(ctx, nbr, attr, perms, z, live, tmax, tmin, 0, m + 1),
                   lambda: be.permtest_extremes(ctx, nbr, attr, perms, z, live, tmax, tmin, -1, 2),
                   lambda: be.permtest_extremes(ctx, nbr, small, perms, z, live, tmax, tmin),
                   lambda: be.permtest_extremes(ctx, small_nbr, small, perms, z, live, tmax, tmin),      # the table has 65 rows
                   lambda: be.counts_from_extremes(ctx, n, m, count, 'neighborhoods', None, live, tmax, tmin, *tail),
                   lambda: be.counts_from_extremes(ctx, n, m, count, 'neighborhoods', z, None, tmax, tmin, *tail),
                   lambda: be.counts_from_extremes(ctx, n, m, count, 'all', z, live, tmax, tmin, None, tail[1], None, None),
                   lambda: be.counts_from_extremes(ctx, n, m, 0, 'all', z, live, tmax, tmin, *tail),
                   lambda: be.counts_from_extremes(ctx, n, m, -3, 'all', z, live, tmax, tmin, *tail),
                   lambda: be.counts_from_extremes(ctx, n, m, count, 2, z, live, tmax, tmin, *tail),
                   lambda: be.counts_from_extremes(ctx, n, m, count, -1, z, live, tmax, tmin, *tail),
                   lambda: be.counts_from_extremes(ctx, 0, m, count, 'all', z, live, tmax, tmin, *tail)]
        for i, call in enumerate(refused):
            with pytest.raises(amd.SafeHipError) as err:
                call()
            assert err.value.code == be._lib.E_INVALID, i
        for name in out.shapes:
            out.read(name, written=False)
    finally:
        out.free()
        perms.close()
        small_nbr.close()
        small.close()
        attr.close()
        nbr.close()
