"""The layer under the enrichment kernels against NumPy, at the sizes where its kernels change path: the whole-matrix
attribute facts (k_attr_stats, k_stats_finish, k_value_census, k_u8_to_f32, k_nan_to_zero of attr.hip), the fused dense
Euclidean kernel in all six instantiations and both loops, the edge lengths, and the membership forms with an accessor
(bit matrix -> dense, row counts, CSR) on both sides of the 4096-column group of k_fill_csr / k_row_popcount.  Inputs and
references: tests/prep_ref.py (self-tested in tests/test_prep_ref_cpu.py).  Every comparison is exact -- integers, bytes or
f64 bit patterns; no tolerance appears in this file.  Needs an MI355X."""
import numpy as np
import pytest

import prep_ref as pr

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (checker only)

STAT_KEYS = ('n_other', 'max_nan_col', 'n_rows_with_value', 'n_non_integer')


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
def torch(amd):
    import torch
    assert torch.cuda.is_available()
    return torch


def same_bits(got, want):
    """Two arrays of one dtype agree byte for byte (NaN payloads and the sign of zero included)."""
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(u), want.view(u))


# ======================================================================================= 1. attribute facts ====

def laid_out(b, order):
    return np.asfortranarray(b) if order == 'F' else np.ascontiguousarray(b)


def open_attr(be, ctx, torch, b, order, way):
    """(handle, what keeps a borrowed buffer alive) for the matrix b through one way in."""
    n, m = b.shape
    if way == 'host':
        return be.Attributes.from_host(ctx, laid_out(b, order)), None
    flat = np.ascontiguousarray(b.T if order == 'F' else b).reshape(-1)          # the bytes of b in `order`
    t = torch.from_numpy(flat).to('cuda')
    torch.cuda.synchronize()
    return be.Attributes.from_device(ctx, t.data_ptr(), b.dtype, n, m, order=order, keepalive=t), t


def check_facts(attr, b, order, what, sums, flags=None):
    """Everything the handle says about its matrix against prep_ref.attr_facts(b); flags: the caller's own row flags."""
    want = pr.attr_facts(b)
    if flags is not None:
        want['row_flags'], want['n_rows_with_value'] = flags, int(flags.sum())
    stats = attr.stats()
    assert stats == {k: want[k] for k in STAT_KEYS}, (what, stats, {k: want[k] for k in STAT_KEYS})
    got_flags = attr.row_flags()
    bad = np.nonzero(got_flags != want['row_flags'])[0]
    assert got_flags.dtype == np.uint8 and bad.size == 0, (what, 'row flags differ at rows', bad[:8].tolist())
    assert attr.value_counts() == want['value_counts'], (what, attr.value_counts(), want['value_counts'])
    assert same_bits(attr.download(b.dtype, order), laid_out(b, order)), (what, 'download')
    got_sums = attr.column_sums()
    assert got_sums.shape == (b.shape[1],) and got_sums.dtype == np.float64
    if sums:                                                            # integers add exactly in any order
        bad = np.nonzero(pr.bits(got_sums) != pr.bits(want['col_sum']))[0]
        assert bad.size == 0, (what, 'column sums differ at columns', bad[:8].tolist(), got_sums[bad[:8]], want['col_sum'][bad[:8]])


VARIANTS = (('binary', False), ('mixed', False), ('binary', True))      # (flavour, one column NaN throughout)


@pytest.mark.parametrize('order,n,m', [('F',) + s for s in pr.F_SHAPES] + [('C',) + s for s in pr.C_SHAPES])
def test_attribute_facts_match_numpy(be, ctx, torch, order, n, m):
    """f32 and f64, 0 / 1 and mixed values, uploaded and borrowed: Fortran order at the edges of the four-row loads
    (n % 4, 1024 rows per wave of loads, 4096 per trip), C order at the edges of the row chunks and column groups."""
    inputs = [(dtype, flavour, nan_column, True) for dtype in (np.float32, np.float64) for flavour, nan_column in VARIANTS]
    if n <= 2:                                                          # (the designed rows leave nothing but NaN there)
        inputs += [(dtype, flavour, False, False) for dtype in (np.float32, np.float64) for flavour in ('binary', 'mixed')]
    for dtype, flavour, nan_column, designed in inputs:
        b = pr.attr_input(n, m, dtype, flavour, seed=3, nan_column=nan_column, designed=designed)
        for way in ('host', 'device'):
            what = '%s %s %s nan_column=%s designed=%s from_%s' % (order, np.dtype(dtype).name, flavour, nan_column, designed, way)
            attr, keep = open_attr(be, ctx, torch, b, order, way)
            try:
                check_facts(attr, b, order, what, sums=flavour == 'binary')
                if nan_column:
                    assert attr.stats()['max_nan_col'] == n
            finally:
                attr.close()


@pytest.mark.parametrize('m,order', pr.LARGE_LAYOUTS)
@pytest.mark.parametrize('n', pr.LARGE_ROWS)
def test_attribute_facts_with_a_dynamic_lds_row_bitmap(be, ctx, torch, n, m, order):
    """The row bitmap at and past the 32 KiB static limit and at its documented ceiling of 150 KiB (1 228 800 rows), f32."""
    for flavour in ('binary', 'mixed'):
        b = pr.attr_input(n, m, np.float32, flavour, seed=4)
        attr, _ = open_attr(be, ctx, torch, b, order, 'host')
        try:
            check_facts(attr, b, order, '%s %d x %d %s' % (order, n, m, flavour), sums=flavour == 'binary')
        finally:
            attr.close()


def test_one_row_past_the_lds_ceiling_is_refused_and_nothing_breaks(amd, be, ctx, torch):
    b = pr.attr_input(pr.ROW_LIMIT + 1, 1, np.float32, 'binary', seed=5)
    attr = be.Attributes.from_host(ctx, b)
    try:
        for call in (attr.stats, attr.row_flags, attr.column_sums):
            with pytest.raises(amd.SafeHipError) as err:
                call()
            assert 'too many rows for the LDS row bitmap' in str(err.value) and err.value.code == be._lib.E_INVALID
        assert attr.value_counts() == pr.attr_facts(b)['value_counts']  # (the census needs no bitmap)
    finally:
        attr.close()                                                    # the handle still closes
    assert attr.handle is None
    small = pr.attr_input(257, 3, np.float32, 'binary', seed=5)
    for order in ('F', 'C'):
        attr, _ = open_attr(be, ctx, torch, small, order, 'host')
        try:
            check_facts(attr, small, order, 'after the refusal, %s' % order, sums=True)
        finally:
            attr.close()


@pytest.mark.parametrize('n,m', pr.U8_SHAPES)
def test_byte_matrices_become_the_f32_matrix(be, ctx, n, m):
    """uint8 and bool uploads (k_u8_to_f32: 16 bytes per thread, a scalar tail) at the element counts around 16 and 4096."""
    for dtype in (np.uint8, np.bool_):
        for order in ('C', 'F'):
            raw = laid_out(pr.attr_input(n, m, dtype, 'binary', seed=6), order)
            b = raw.astype(np.float32)
            attr = be.Attributes.from_host(ctx, raw)
            try:
                check_facts(attr, b, order, '%s %s' % (np.dtype(dtype).name, order), sums=True)
            finally:
                attr.close()
    if n * m >= 255:
        raw = (np.arange(n * m).reshape(n, m) % 256).astype(np.uint8)   # every byte value, in place
        attr = be.Attributes.from_host(ctx, raw)
        try:
            check_facts(attr, raw.astype(np.float32), 'C', 'all byte values', sums=True)
        finally:
            attr.close()


TRANSITION_SHAPES = (('F', 4097, 3), ('F', 70, 130), ('F', 5, 1), ('C', 257, 65), ('C', 4097, 2), ('C', 17, 130))


@pytest.mark.parametrize('order,n,m', TRANSITION_SHAPES)
def test_nan_to_zero_then_all_facts_again(be, ctx, torch, order, n, m):
    for dtype in (np.float32, np.float64):
        for flavour in ('binary', 'mixed'):
            b = pr.attr_input(n, m, dtype, flavour, seed=7)
            for way in ('host', 'device'):
                what = '%s %s from_%s' % (np.dtype(dtype).name, flavour, way)
                attr, keep = open_attr(be, ctx, torch, b, order, way)
                try:
                    check_facts(attr, b, order, what + ' before', sums=flavour == 'binary')     # (fills every lazy cache)
                    before = attr.column_sums()
                    attr.nan_to_zero()
                    zeroed = np.where(np.isnan(b), dtype(0), b)
                    check_facts(attr, zeroed, order, what + ' after', sums=flavour == 'binary')
                    assert attr.stats()['max_nan_col'] == 0 and attr.value_counts()[0] == 0
                    assert attr.row_flags().all() and attr.stats()['n_rows_with_value'] == n
                    if flavour == 'binary':
                        assert np.array_equal(pr.bits(attr.column_sums()), pr.bits(before))
                    if way == 'device':                                 # in place: the caller's buffer is the matrix
                        torch.cuda.synchronize()
                        mine = keep.cpu().numpy().reshape((m, n) if order == 'F' else (n, m))
                        assert same_bits(np.ascontiguousarray(mine.T if order == 'F' else mine), np.ascontiguousarray(zeroed))
                finally:
                    attr.close()


@pytest.mark.parametrize('order,n,m', TRANSITION_SHAPES)
def test_row_flags_set_before_the_first_statistics_pass_are_kept(be, ctx, torch, order, n, m):
    for dtype in (np.float32, np.float64):
        for flavour in ('binary', 'mixed'):
            b = pr.attr_input(n, m, dtype, flavour, seed=8)
            flags = (np.random.default_rng(n + m).uniform(size=n) < 0.5).astype(np.uint8)
            flags[:2] = (1, 0)                                          # row 0 is all NaN and flagged; row 1 has a value and is not
            attr, _ = open_attr(be, ctx, torch, b, order, 'host')
            try:
                attr.set_row_flags(flags)
                check_facts(attr, b, order, '%s %s' % (np.dtype(dtype).name, flavour), sums=flavour == 'binary', flags=flags[:n])
            finally:
                attr.close()


# ================================================================== 2. the fused dense Euclidean kernel ====

@pytest.fixture(scope='module')
def dense_sizes(ctx):
    nb, sizes = pr.dense_sizes(ctx.num_cu)
    if nb is None or nb > 4100:
        pytest.fail('k_euclid_dense runs whole batches only from n = %s on with %d compute units: the [n, n] outputs of this '
                    'test would no longer be small -- choose the sizes anew' % (nb, ctx.num_cu))
    return nb, sizes


def test_the_sizes_reach_both_loops_and_a_single_column_lane(ctx, dense_sizes):
    nb, sizes = dense_sizes
    print('compute units %d: first n with whole batches %d; sizes %s' % (ctx.num_cu, nb, sizes))
    batched = [n for n in sizes.values() if pr.dense_geometry(n, ctx.num_cu)[2]]
    assert batched and {n % 2 for n in batched} == {0, 1}, 'no size runs whole batches in both store forms'
    assert any(not pr.dense_geometry(n, ctx.num_cu)[2] for n in sizes.values())
    assert any(pr.last_lane_has_one_column(n) for n in sizes.values()), 'no size has a last lane with a single column'
    assert len({pr.dense_geometry(n, ctx.num_cu)[0] for n in sizes.values()}) >= 4


def run_dense(ctx, xy, nr, want_mask, want_dist):
    """safe_euclidean_dense_dev into sentinel-filled device buffers (-1 / NaN: a stale or unwritten entry cannot pass);
    want_* None: that output is not requested."""
    n = xy.shape[0]
    d_xy = ctx.alloc(xy.nbytes)
    d_xy.upload(xy)
    d_mask = d_dist = None
    try:
        if want_mask is not None:
            d_mask = ctx.alloc(n * n * 8)
            d_mask.upload(np.full((n, n), -1, dtype=np.int64))
        if want_dist is not None:
            d_dist = ctx.alloc(n * n * 8)
            d_dist.upload(np.full((n, n), np.nan))
        ctx.euclidean_dense(d_xy.ptr, n, nr, d_mask.ptr if d_mask else None, d_dist.ptr if d_dist else None)
        ctx.sync()
        mode = '%s%s' % ('mask' if d_mask else '', 'dist' if d_dist else '')
        if d_mask:
            got = d_mask.download((n, n), np.int64)
            bad = np.argwhere(got != want_mask)
            assert bad.shape[0] == 0, (mode, n, '%d mask entries differ, first at' % bad.shape[0], bad[:4].tolist(),
                                       [int(got[i, j]) for i, j in bad[:4]])
        if d_dist:
            got = d_dist.download((n, n), np.float64)
            bad = np.argwhere(pr.bits(got) != pr.bits(want_dist))
            assert bad.shape[0] == 0, (mode, n, '%d distances differ, first at' % bad.shape[0], bad[:4].tolist(),
                                       [float(got[i, j]) for i, j in bad[:4]])
    finally:
        for d in (d_xy, d_mask, d_dist):
            if d is not None:
                d.free()


@pytest.mark.parametrize('slot', pr.DENSE_SLOTS)
@pytest.mark.parametrize('kind', pr.XY_KINDS)
def test_dense_kernel_every_mode_against_pdist(ctx, dense_sizes, kind, slot):
    """Mask only, distances only, both -- with odd and even n the six instantiations -- below, at and past the first n that
    enters the whole-batch loop.  'tiny': the mask alone (its claim is the squared threshold, which takes no device root)."""
    n = dense_sizes[1][slot]
    xy = pr.xy_input(kind, n)
    nr = pr.XY_RADIUS[kind]
    want_d = orc.euclidean_distances(xy)
    want_m = (want_d < nr).astype(np.int64)
    if n > 10:
        assert want_m[0, 1] == 1 and want_d[2, 3] == nr and want_m[2, 3] == 0       # the coincident pair; the pair on the threshold
    run_dense(ctx, xy, nr, want_m, None)
    if kind != 'tiny':
        run_dense(ctx, xy, nr, None, want_d)
        run_dense(ctx, xy, nr, want_m, want_d)


RADIUS_NAMES = ('zero', 'negative', 'nan', 'inf', '1e200', '1e-200', 'smallest_subnormal', 'default')


@pytest.mark.parametrize('which', range(len(RADIUS_NAMES)), ids=RADIUS_NAMES)
@pytest.mark.parametrize('kind', ['uniform', 'tiny', 'huge'])
def test_radius_edges_in_both_euclidean_kernels(be, ctx, kind, which):
    """Expected membership is pdist < nr.  On 'tiny' every squared distance and most thresholds are subnormal: the device
    must compare subnormal doubles without flushing them."""
    n = 300
    xy = pr.xy_input(kind, n)
    nr = pr.radius_edges(xy)[which]
    want = (orc.euclidean_distances(xy) < nr).astype(np.int64)
    if RADIUS_NAMES[which] in ('zero', 'negative', 'nan'):
        assert want.sum() == 0
    elif RADIUS_NAMES[which] != 'default' or kind == 'uniform':
        assert want[0, 1] == 1 and want.trace() == n                    # the coincident pair and the diagonal
    if kind == 'tiny' and RADIUS_NAMES[which] == 'default':
        assert n < want.sum() < n * n                                   # a threshold in the middle of the subnormal squares
    run_dense(ctx, xy, nr, want, None)
    nbr = be.Neighborhoods.euclidean(ctx, xy, nr)
    try:
        check_forms(nbr, want, None, 'euclidean %s nr=%r' % (kind, nr))
    finally:
        nbr.close()


@pytest.mark.parametrize('n_edges', [0, 1, 255, 256, 257])
@pytest.mark.parametrize('kind', ['uniform', 'lattice', 'offset'])
def test_edge_lengths_match_the_oracle_bit_for_bit(ctx, kind, n_edges):
    xy = pr.xy_input(kind, 300)
    eu, ev = pr.edge_input(300, n_edges)
    got = ctx.edge_lengths(xy, eu, ev)
    want = orc.edge_lengths(xy, eu, ev)
    assert got.shape == (n_edges,) and np.array_equal(pr.bits(got), pr.bits(want))
    if n_edges:
        assert got[0] == 0.0                                            # the self edge
    if n_edges >= 3:
        assert got[-1] == got[1]                                        # the repeated edge


# ================================================================================= 3. membership forms ====

def check_forms(nbr, a, torch, what):
    """Every form of the handle that has a way out against the dense 0 / 1 matrix a (torch None: no device-side copy)."""
    n = a.shape[0]
    counts = a.sum(axis=1)
    assert (nbr.n, nbr.nnz, nbr.max_row_count) == (n, int(a.sum()), int(counts.max())), (what, nbr.n, nbr.nnz, nbr.max_row_count)
    got = nbr.to_dense()
    bad = np.argwhere(got != a)
    assert got.dtype == np.int64 and bad.shape[0] == 0, (what, 'to_dense differs at', bad[:4].tolist())
    if torch is not None:
        t = torch.full((n, n), -1, dtype=torch.int64, device='cuda')    # a sentinel no membership has
        torch.cuda.synchronize()
        nbr.to_dense_dev(t.data_ptr())
        nbr.ctx.sync()
        assert np.array_equal(t.cpu().numpy(), a), (what, 'to_dense_dev')
    got_counts = nbr.row_counts()
    bad = np.nonzero(got_counts != counts)[0]
    assert bad.size == 0, (what, 'row counts differ at rows', bad[:8].tolist(), got_counts[bad[:8]], counts[bad[:8]])
    row_ptr, col = nbr.csr()
    want_ptr, want_col = pr.csr_of(a)
    assert row_ptr.dtype == col.dtype == np.int32
    assert np.array_equal(row_ptr, want_ptr), (what, 'row_ptr')
    bad = np.nonzero(col != want_col)[0] if col.shape == want_col.shape else np.arange(1)
    if bad.size:
        row = int(np.searchsorted(want_ptr, bad[0], side='right') - 1)
        assert False, (what, 'CSR columns differ from np.nonzero, first in row %d at entry %d of it' % (row, bad[0] - want_ptr[row]),
                       col[bad[0]:bad[0] + 4].tolist(), want_col[bad[0]:bad[0] + 4].tolist())


@pytest.mark.parametrize('n', pr.MEMBERSHIP_SIZES)
def test_membership_forms_match_np_nonzero(be, ctx, torch, n):
    """from_dense of the designed matrix: odd n takes the scalar store of k_bits_to_dense and even n the pair store; from
    4097 columns on a row spans two 64-word groups, and the CSR offsets of the second depend on the carry out of the first."""
    a = pr.membership(n)
    nbr = be.Neighborhoods.from_dense(ctx, a)
    try:
        check_forms(nbr, a, torch, 'from_dense n=%d' % n)
    finally:
        nbr.close()


@pytest.mark.parametrize('how', ['zeros_1', 'zeros_65', 'euclidean_0'])
def test_empty_memberships_are_empty_in_every_form(be, ctx, torch, how):
    n = 1 if how == 'zeros_1' else 65
    if how == 'euclidean_0':
        nbr = be.Neighborhoods.euclidean(ctx, pr.xy_input('uniform', n), 0.0)
    else:
        nbr = be.Neighborhoods.from_dense(ctx, np.zeros((n, n), dtype=np.int64))
    try:
        check_forms(nbr, np.zeros((n, n), dtype=np.int64), torch, how)
        row_ptr, col = nbr.csr()
        assert nbr.nnz == 0 and nbr.max_row_count == 0 and not row_ptr.any() and row_ptr.shape == (n + 1,) and col.shape == (0,)
    finally:
        nbr.close()


@pytest.mark.parametrize('n', [65, 129])
def test_values_outside_0_and_1_are_refused_wherever_they_sit(amd, be, ctx, torch, n):
    """The corners of the matrix and of its words: first and last lane of the first and of the last (ragged) word of a row."""
    a = pr.membership(n)
    for value in (2, -1):
        for i, j in ((0, 0), (0, 64), (n - 1, n - 1), (n - 1, 63)):
            bad = a.copy()
            bad[i, j] = value
            with pytest.raises(amd.SafeHipError) as err:
                be.Neighborhoods.from_dense(ctx, bad)
            assert err.value.code == be._lib.E_VALUE and 'entries outside {0,1}' in str(err.value), (value, i, j)
    nbr = be.Neighborhoods.from_dense(ctx, a)                           # and a valid handle afterwards is correct
    try:
        check_forms(nbr, a, torch, 'after the refusals')
    finally:
        nbr.close()


def test_euclidean_membership_past_4096_columns(be, ctx, torch):
    """The bit-matrix route of safe_nbr_euclidean at 4161 lattice nodes: rows of up to several thousand members on both
    sides of column 4096."""
    n = 4161
    xy = pr.xy_input('lattice', n)
    nr = 40.0
    want = (orc.euclidean_distances(xy) < nr).astype(np.int64)
    counts = want.sum(axis=1)
    assert counts.max() > 3000 and (want[:, :4096].any(axis=1) & want[:, 4096:].any(axis=1)).sum() > 1000
    nbr = be.Neighborhoods.euclidean(ctx, xy, nr)
    try:
        check_forms(nbr, want, torch, 'euclidean lattice n=%d' % n)
    finally:
        nbr.close()
