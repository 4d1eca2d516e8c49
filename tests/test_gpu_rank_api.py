"""SAFE.compute_pvalues(attribute_transform='rank'): the device-ranked run against a second instance whose host matrix was
ranked with SciPy first -- every result bit for bit, for the analytic test and for the seeded randomization test -- and the
Mann-Whitney identity of the analytic test on ranks.

The host-ranked matrix is handed over in Fortran order, the order of the ranked handle: safe_attr_rank promises a handle that
no later call can tell from safe_attr_create_host of R in that order, and the centred sums of squares of the analytic test
add up in an order that follows the element order.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, RADIUS, SEED, NPERM = 300, 40, 0.12, 7, 100
RESULTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')

# Mann-Whitney identity: the largest relative difference between scipy's tie-corrected asymptotic z and the analytic z that the
# code before this feature gives on the host-ranked column (measured with measure_mann_whitney_gap below on an MI355X), and the
# factor the two routes are allowed -- they add in different orders.
MW_MEASURED = 2.98e-16
MW_ALLOWED = 4 * MW_MEASURED


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def data():
    return make_data()


def make_data():
    """(xy, B): 300 nodes, 40 quantitative columns -- rounded values (ties), heavy tails, 0/1 and constant columns, NaN cells,
    three rows without any value, one column that is mostly NaN."""
    rng = np.random.default_rng(300)
    xy = rng.uniform(size=(N, 2))
    b = np.round(rng.standard_t(2, size=(N, M)), 1)
    b[:, 3] = rng.uniform(size=N) < 0.2
    b[:, 4] = 2.5
    b[:, 5] = rng.normal(size=N)                                # distinct values
    b[rng.uniform(size=(N, M)) < 0.05] = np.nan
    b[rng.uniform(size=N) < 0.6, 6] = np.nan
    b[[10, 11, 250]] = np.nan
    b.flags.writeable = False
    xy.flags.writeable = False
    return xy, b


def host_ranked(b):
    from scipy.stats import rankdata
    return np.asfortranarray(rankdata(b, method='average', axis=0, nan_policy='omit'))


def make(amd, xy, attributes, **load):
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(np.array(xy))
    sf.random_seed = SEED
    sf.num_permutations = NPERM
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=RADIUS)
    sf.load_attributes(attribute_file=attributes, **load)
    return sf


def assert_same_results(got, want):
    for name in RESULTS:
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.shape == b.shape == (N, M) and np.array_equal(a, b, equal_nan=True), name
    assert np.array_equal(got.attributes['num_neighborhoods_enriched'].values, want.attributes['num_neighborhoods_enriched'].values)


@pytest.fixture(scope='module')
def pair(amd, data):
    """(instance on the raw matrix, instance on the host-ranked matrix), reused by the cases that change nothing but a keyword."""
    xy, b = data
    return make(amd, xy, np.array(b)), make(amd, xy, host_ranked(b))


def test_neighborhoods_have_several_sizes(pair):
    sizes = np.unique(pair[0].neighborhoods.sum(axis=1))
    assert len(sizes) >= 10 and sizes.min() >= 1


@pytest.mark.parametrize('multiple_testing', [False, True])
def test_analytic_on_device_ranks_equals_analytic_on_host_ranks(pair, data, multiple_testing):
    raw, ranked = pair
    raw.compute_pvalues(how='analytic', attribute_transform='rank', multiple_testing=multiple_testing)
    ranked.compute_pvalues(how='analytic', attribute_transform='none', multiple_testing=multiple_testing)
    assert_same_results(raw, ranked)
    assert np.array_equal(raw.node2attribute, data[1], equal_nan=True)                # the raw matrix is not touched
    r = host_ranked(data[1])
    a = raw.neighborhoods.astype(np.float64)
    assert np.array_equal(np.asarray(raw.ns), a @ np.nan_to_num(r))                    # rank sums (half-integers: exact)
    assert np.asarray(raw.nes_binary).sum() > 0


@pytest.mark.parametrize('score', ['sum', 'z-score'])
def test_randomization_on_device_ranks_equals_randomization_on_host_ranks(pair, score):
    raw, ranked = pair
    raw.compute_pvalues(how='randomization', neighborhood_score_type=score, attribute_transform='rank', multiple_testing=False)
    ranked.compute_pvalues(how='randomization', neighborhood_score_type=score, attribute_transform='none', multiple_testing=False)
    assert_same_results(raw, ranked)
    raw.neighborhood_score_type = ranked.neighborhood_score_type = 'sum'


def test_auto_looks_at_the_raw_values(pair):
    raw, ranked = pair
    raw.compute_pvalues(how='auto', neighborhood_score_type='sum', attribute_transform='rank', multiple_testing=False)
    ranked.compute_pvalues(how='randomization', neighborhood_score_type='sum', attribute_transform='none', multiple_testing=False)
    assert_same_results(raw, ranked)


def test_background_network(amd, data):
    xy, b = data
    raw = make(amd, xy, np.array(b))
    raw.compute_pvalues(how='analytic', attribute_transform='rank', background='network')
    ranked = make(amd, xy, host_ranked(np.nan_to_num(b)))       # NaN -> 0 first, then the ranks (the zeros tie)
    ranked.compute_pvalues(how='analytic')
    assert_same_results(raw, ranked)
    assert np.array_equal(raw.node2attribute, np.nan_to_num(b))  # background = 'network' edits the host matrix, as without the transform


def test_sparse_input(amd, data):
    import scipy.sparse as sp
    xy, b = data
    dense = np.where(np.abs(np.nan_to_num(b)) > 1.0, np.nan_to_num(b), 0.0)
    missing = np.isnan(b).all(axis=1)
    dense[missing] = 0.0
    raw = make(amd, xy, sp.csc_matrix(dense), missing_rows=missing)
    raw.compute_pvalues(how='analytic', attribute_transform='rank')
    full = dense.copy()
    full[missing] = np.nan
    ranked = make(amd, xy, host_ranked(full))
    ranked.compute_pvalues(how='analytic')
    assert_same_results(raw, ranked)
    assert sp.issparse(raw.node2attribute) and np.array_equal(raw.node2attribute.toarray(), dense)


def test_none_is_the_call_without_the_keyword(amd, data):
    xy, b = data
    with_kw, without = make(amd, xy, np.array(b)), make(amd, xy, np.array(b))
    for how in ('analytic', 'randomization'):
        with_kw.compute_pvalues(how=how, attribute_transform='none')
        without.compute_pvalues(how=how)
        assert_same_results(with_kw, without)
    assert without.attribute_transform == 'none'


def test_resident_handle_and_host_matrix_are_untouched(amd, data):
    xy, b = data
    host = np.array(b)
    sf = make(amd, xy, host, keep_on_device=True)
    resident = sf._attr_dev
    assert resident is not None
    sf.compute_pvalues(how='analytic', attribute_transform='rank')
    assert sf._attr_dev is resident and resident.handle
    assert np.array_equal(resident.download(np.float64, order='C'), b, equal_nan=True)
    assert sf.node2attribute is host and np.array_equal(host, b, equal_nan=True)
    ranked = make(amd, xy, host_ranked(b))
    ranked.compute_pvalues(how='analytic')
    assert_same_results(sf, ranked)
    sf.compute_pvalues(how='analytic', attribute_transform='none')                    # and the raw test still runs on the raw values
    # (sums of raw values: the suite's tolerance for observed scores, tests/test_gpu_stream_order.py)
    assert np.allclose(np.asarray(sf.ns), sf.neighborhoods.astype(np.float64) @ np.nan_to_num(b), rtol=1e-9, atol=1e-12)


def test_refusals_write_no_result(amd, data):
    xy, b = data
    binary = (np.nan_to_num(b) > 1.0).astype(np.float64)
    sf = make(amd, xy, binary)
    for how in ('hypergeometric', 'auto'):
        with pytest.raises(ValueError, match='ranks are not counts'):
            sf.compute_pvalues(how=how, attribute_transform='rank')
        for name in RESULTS:
            assert getattr(sf, name) is None, (how, name)
        assert 'num_neighborhoods_enriched' not in sf.attributes
    with pytest.raises(ValueError, match='attribute_transform'):
        sf.compute_pvalues(how='analytic', attribute_transform='ranks')
    assert sf.attribute_transform == 'none' and sf.ns is None
    sf.compute_pvalues(how='auto')                              # the same instance still works: the hypergeometric test of 0/1 data
    assert sf.pvalues_pos is not None


def mann_whitney_gap(amd, xy, column, ranked_handle, rows):
    """Largest relative difference, over the neighborhoods `rows`, between the z of the analytic test on the ranked column and
    scipy.stats.mannwhitneyu(members, others, method='asymptotic', use_continuity=False)'s U turned into z with the
    tie-corrected variance n1 n2 / 12 ((n + 1) - sum(t^3 - t) / (n (n - 1)))."""
    from scipy.stats import mannwhitneyu
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    n = column.shape[0]
    r = float(RADIUS * (xy[:, 0].max() - xy[:, 0].min()))
    nbr = be.Neighborhoods.euclidean(ctx, np.array(xy), r)
    bufs = [ctx.alloc_f64(n) for _ in range(5)] + [ctx.alloc_f64(1), ctx.alloc_f64(n)]
    try:
        a = nbr.to_dense().astype(bool)
        be.moments_test(ctx, nbr, ranked_handle, 'both', 0.05, [x.ptr for x in bufs[:6]], z_ptr=bufs[6].ptr)
        z = bufs[6].download((n,))
    finally:
        for x in bufs:
            x.free()
        nbr.close()
    _, counts = np.unique(column, return_counts=True)
    ties = float((counts.astype(np.float64) ** 3 - counts).sum())
    gap = 0.0
    for i in rows:
        x, y = column[a[i]], column[~a[i]]
        n1, n2 = len(x), len(y)
        assert n1 >= 2 and n2 >= 2
        u = mannwhitneyu(x, y, method='asymptotic', use_continuity=False).statistic
        var = n1 * n2 / 12.0 * ((n + 1) - ties / (n * (n - 1.0)))
        z_ref = (u - n1 * n2 / 2.0) / np.sqrt(var)
        assert abs(z_ref) > 1e-3                                # (a relative difference means something)
        gap = max(gap, abs(z[i] - z_ref) / abs(z_ref))
    return gap


MW_ROWS = (0, 17, 99, 123, 200, 299)


def mw_column(data):
    return np.ascontiguousarray(np.round(np.random.default_rng(5).standard_t(2, size=N), 1))      # NaN-free, ties, heavy tails


def measure_mann_whitney_gap(amd, data):
    """The figure MW_MEASURED records: the analytic z of the HOST-ranked column (code that knows no transform) against SciPy."""
    from safepy_amd import backend as be
    col = mw_column(data)
    handle = be.Attributes.from_host(be.Context.default(0), host_ranked(col[:, None]))
    try:
        return mann_whitney_gap(amd, data[0], col, handle, MW_ROWS)
    finally:
        handle.close()


def test_analytic_z_of_ranks_is_the_mann_whitney_z(amd, data):
    """The analytic test on device ranks is the tie-corrected Mann-Whitney test: its z against SciPy's U, six neighborhoods of
    a NaN-free column with ties.  Tolerance 4 x the difference measured for the analytic test on the host-ranked column with
    the code before this feature: MW_MEASURED = 2.98e-16 relative (the two routes add in different orders; at most a few
    roundings of a double)."""
    from safepy_amd import backend as be
    col = mw_column(data)
    src = be.AttributeMatrix.from_host(be.Context.default(0), col[:, None])
    ranked = src.rank()
    try:
        gap = mann_whitney_gap(amd, data[0], col, ranked, MW_ROWS)
    finally:
        ranked.close()
        src.close()
    print('Mann-Whitney identity: largest relative difference %.3g (allowed %.3g)' % (gap, MW_ALLOWED))
    assert gap <= MW_ALLOWED
