"""SAFE.compute_pvalues(multiple_testing=True, multiple_testing_scope=...) on the device, every route that honours
multiple_testing: the adjusted p matrices equal the oracle's Benjamini-Hochberg along the scope of the SAME call's unadjusted
matrices on the bits, and nes / nes_binary / num_neighborhoods_enriched equal the pinned epilogues (safe_hypergeom_outputs for the
two-sided routes, safe_fdr_adjust on the expected matrix reshaped to [N M, 1] for the others) applied to those expected p-values.
N = 257 nodes, M = 70 attributes, Euclidean neighborhoods, random_seed = 0.  Needs an MI355X."""
import numpy as np
import pytest

import fdr_cases as fc
import fdr_scope_ref as fs

pytestmark = pytest.mark.gpu

N, M, RADIUS, THRESHOLD = 257, 70, 0.15, 0.05
SCOPES = ('attributes', 'neighborhoods', 'all')
SIGNS = ('highest', 'lowest', 'both')
BIG_P = fs.ALL_HIST_MAX_P + 17              # beyond the count form of every scope (rows 5119, columns 4095, matrix 16383)

# name -> (compute_pvalues keywords, attribute kind, two-sided epilogue?)
ROUTES = {
    'binary-P100': (dict(how='randomization', num_permutations=100), 'binary', False),
    'zscore-P100': (dict(how='randomization', num_permutations=100, neighborhood_score_type='z-score'), 'quantitative', False),
    'binary-bigP': (dict(how='randomization', num_permutations=BIG_P), 'binary', False),
    'hypergeom-upper': (dict(how='hypergeometric', hypergeom_tails='upper'), 'binary', False),
    'hypergeom-sign': (dict(how='hypergeometric', hypergeom_tails='attribute_sign'), 'binary', True),
    'analytic': (dict(how='analytic'), 'quantitative', True),
    'analytic-rank': (dict(how='analytic', attribute_transform='rank'), 'quantitative', True),
}
CASES = [(route, sign) for route in ROUTES for sign in (SIGNS if route != 'hypergeom-upper' else ('highest',))]


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
def data():
    rng = np.random.default_rng(0)
    xy = rng.uniform(size=(N, 2))
    binary = (rng.uniform(size=(N, M)) < 0.15).astype(np.float64)
    near = np.hypot(xy[:, 0] - 0.5, xy[:, 1] - 0.5) < 0.2
    binary[near, :5] = (rng.uniform(size=(int(near.sum()), 5)) < 0.7).astype(np.float64)      # enrichment that survives adjustment
    quantitative = rng.normal(size=(N, M))
    quantitative[near, :5] += 2.0
    return {'xy': xy, 'binary': binary, 'quantitative': quantitative}


def make(amd, data, kind, sign, lazy=True):
    sf = amd.SAFE(verbose=False)
    sf.lazy_outputs = lazy
    sf.graph = amd.LayoutGraph(data['xy'])
    sf.random_seed = 0
    sf.attribute_sign = sign
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=RADIUS)
    sf.load_attributes(attribute_file=(data[kind] if isinstance(kind, str) else kind).copy())
    return sf


def results(sf):
    out = {key: (None if getattr(sf, key) is None else np.array(getattr(sf, key), dtype=np.float64))
           for key in ('pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')}
    out['num_neighborhoods_enriched'] = np.asarray(sf.attributes['num_neighborhoods_enriched'], dtype=np.float64)
    return out


def run(sf, keywords, **more):
    sf.ns = sf.pvalues_neg = sf.pvalues_pos = sf.nes = sf.nes_binary = None
    sf.compute_pvalues(**dict(keywords, **more))
    return results(sf)


def pinned_epilogue(be, ctx, two_sided, q_neg, q_pos, num_permutations, sign):
    """(nes, nes_binary, num_enriched) of the existing epilogues on expected adjusted p-values."""
    n, m = q_pos.shape
    if two_sided:
        bufs = [ctx.alloc_f64(n, m) for _ in range(4)] + [ctx.alloc_f64(m)]
        try:
            bufs[0].upload(q_neg)
            bufs[1].upload(q_pos)
            be.hypergeom_outputs(ctx, n, m, sign, THRESHOLD, bufs[0].ptr, bufs[1].ptr, [b.ptr for b in bufs[2:]])
            return bufs[2].download((n, m)), bufs[3].download((n, m)), bufs[4].download((m,))
        finally:
            for b in bufs:
                b.free()
    bufs = [ctx.alloc_f64(n * m, 1) for _ in range(4)] + [ctx.alloc_f64(1)]
    try:
        if q_neg is not None:
            bufs[0].upload(q_neg.reshape(-1, 1))
        bufs[1].upload(q_pos.reshape(-1, 1))
        be.fdr_adjust(ctx, n * m, 1, num_permutations, sign, THRESHOLD, [bufs[0].ptr if q_neg is not None else None] + [b.ptr for b in bufs[1:]])
        assert fc.same(bufs[1].download((n, m)), q_pos)             # a family of one is left as it is
        nes_binary = bufs[3].download((n, m))
        return bufs[2].download((n, m)), nes_binary, nes_binary.sum(axis=0)
    finally:
        for b in bufs:
            b.free()


def canonical(q):
    """The oracle's result with every NaN as the device writes it (0x7FF8...): the epilogue then sees the device's own bits."""
    q = np.ascontiguousarray(q).copy()
    q[np.isnan(q)] = np.float64('nan')
    return q


@pytest.mark.parametrize('route,sign', CASES, ids=['%s-%s' % c for c in CASES])
def test_every_route_and_scope(amd, be, data, route, sign):
    keywords, kind, two_sided = ROUTES[route]
    sf = make(amd, data, kind, sign)
    ctx = sf._ctx()
    plain = run(sf, keywords, multiple_testing=False)
    assert not np.isnan(plain['pvalues_pos']).any()
    num_permutations = keywords.get('num_permutations', 0)
    default = run(sf, keywords, multiple_testing=True)             # no keyword: the reference's rows
    seen = {}
    for scope in SCOPES:
        got = run(sf, keywords, multiple_testing=True, multiple_testing_scope=scope)
        assert sf.multiple_testing_scope == scope
        q_pos = fs.want(plain['pvalues_pos'], scope)
        q_neg = fs.want(plain['pvalues_neg'], scope) if plain['pvalues_neg'] is not None else None
        assert fc.same(got['pvalues_pos'], q_pos), (route, sign, scope)
        if q_neg is not None:
            assert fc.same(got['pvalues_neg'], q_neg), (route, sign, scope)
        nes, nes_binary, enriched = pinned_epilogue(be, ctx, two_sided, None if q_neg is None else canonical(q_neg), canonical(q_pos),
                                                    num_permutations, sign)
        assert np.array_equal(fc.bits(got['nes']), fc.bits(nes)), (route, sign, scope)
        assert np.array_equal(got['nes_binary'], nes_binary), (route, sign, scope)
        assert np.array_equal(got['num_neighborhoods_enriched'], enriched), (route, sign, scope)
        seen[scope] = got
    for key, value in default.items():                               # 'attributes' is byte-equal to a call without the keyword
        other = seen['attributes'][key]
        assert (value is None and other is None) or np.array_equal(fc.bits(value), fc.bits(other)), key
    assert not fc.same(seen['attributes']['pvalues_pos'], seen['neighborhoods']['pvalues_pos'])
    assert not fc.same(seen['attributes']['pvalues_pos'], seen['all']['pvalues_pos'])


@pytest.mark.parametrize('scope', SCOPES[1:])
@pytest.mark.parametrize('route', ['binary-P100', 'hypergeom-upper', 'analytic'])
def test_lazy_outputs_on_and_off_agree_and_results_stay_resident(amd, data, route, scope):
    from safepy_amd.safe import _DeviceResult
    keywords, kind, _ = ROUTES[route]
    lazy, eager = make(amd, data, kind, 'highest', lazy=True), make(amd, data, kind, 'highest', lazy=False)
    eager_out = run(eager, keywords, multiple_testing=True, multiple_testing_scope=scope)
    lazy.compute_pvalues(multiple_testing=True, multiple_testing_scope=scope, **keywords)
    assert all(isinstance(lazy.__dict__.get(slot), _DeviceResult) for slot in ('_r_nes', '_r_nes_binary'))
    pairs = lazy.enriched_pairs(format='coo')
    assert all(isinstance(lazy.__dict__.get(slot), _DeviceResult) for slot in ('_r_nes', '_r_nes_binary'))   # still on the device
    lazy_out = results(lazy)
    rows, cols = np.nonzero(lazy_out['nes_binary'])
    assert np.array_equal(pairs.row, rows) and np.array_equal(pairs.col, cols) and rows.size > 0
    assert np.array_equal(fc.bits(pairs.data), fc.bits(lazy_out['nes'][rows, cols]))
    for key, value in eager_out.items():
        assert (value is None and lazy_out[key] is None) or np.array_equal(fc.bits(value), fc.bits(lazy_out[key])), key


def test_one_clustered_attribute_among_null_attributes(amd, data):
    """Attribute 0 is 1 on one tight cluster of nodes and nowhere else; the other 69 attributes are null (sparse random ones).
    The three host statements give three different numbers of enriched neighborhoods for attribute 0 -- computed here from the
    oracle on the unadjusted matrix, not hard-coded -- and each scope returns its own."""
    rng = np.random.default_rng(7)
    xy = data['xy']
    b = (rng.uniform(size=(N, M)) < 0.08).astype(np.float64)
    b[:, 0] = (np.hypot(xy[:, 0] - 0.5, xy[:, 1] - 0.5) < 0.12).astype(np.float64)
    assert 5 <= b[:, 0].sum() <= 40
    keywords = dict(how='hypergeometric', hypergeom_tails='upper')
    sf = make(amd, data, b, 'highest')
    plain = run(sf, keywords, multiple_testing=False)
    counts, host = {}, {}
    for scope in SCOPES:
        got = run(sf, keywords, multiple_testing=True, multiple_testing_scope=scope)
        q = fs.want(plain['pvalues_pos'], scope)
        with np.errstate(divide='ignore'):
            host[scope] = int((-np.log10(q[:, 0]) > -np.log10(THRESHOLD)).sum())
        counts[scope] = int(got['num_neighborhoods_enriched'][0])
        assert counts[scope] == int(got['nes_binary'][:, 0].sum())
    assert counts == host, (counts, host)
    assert len(set(host.values())) == 3, host                       # the three scopes differ on this input
