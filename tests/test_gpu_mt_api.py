"""SAFE.compute_pvalues(multiple_testing=True, multiple_testing_method=...) on the device, every route that honours
multiple_testing: the adjusted p matrices equal the NumPy restatement tests/mt_ref.py applied, along the scope, to the SAME call's
unadjusted matrices -- on the bits -- and nes / nes_binary / num_neighborhoods_enriched equal the pinned epilogues applied to
those expected p-values (the helpers of tests/test_gpu_fdr_scope_api.py: N = 257 nodes, M = 70 attributes, Euclidean
neighborhoods, random_seed = 0).  Needs an MI355X."""
import pickle

import numpy as np
import pytest

import fdr_cases as fc
import maxt_ref as mx
import mt_ref as mt
import test_gpu_fdr_scope_api as api

pytestmark = pytest.mark.gpu

SCOPES = api.SCOPES
# the hypergeometric route, hypergeom_tails = 'attribute_sign', how = 'analytic', seeded randomization flat and weighted
ROUTES = {name: api.ROUTES[name] for name in ('hypergeom-upper', 'hypergeom-sign', 'analytic', 'binary-P100')}
ROUTES['weighted-P100'] = (dict(how='randomization', num_permutations=100), 'quantitative', False)
SIGN = {'hypergeom-upper': 'highest', 'hypergeom-sign': 'both', 'analytic': 'lowest', 'binary-P100': 'both', 'weighted-P100': 'highest'}


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
    xy = rng.uniform(size=(api.N, 2))
    binary = (rng.uniform(size=(api.N, api.M)) < 0.15).astype(np.float64)
    near = np.hypot(xy[:, 0] - 0.5, xy[:, 1] - 0.5) < 0.2
    binary[near, :5] = (rng.uniform(size=(int(near.sum()), 5)) < 0.7).astype(np.float64)
    quantitative = rng.normal(size=(api.N, api.M))
    quantitative[near, :5] += 2.0
    return {'xy': xy, 'binary': binary, 'quantitative': quantitative}


def make(amd, data, route, lazy=True):
    kind = ROUTES[route][1]
    if route != 'weighted-P100':
        return api.make(amd, data, kind, SIGN[route], lazy)
    sf = amd.SAFE(verbose=False)
    sf.lazy_outputs = lazy
    sf.graph = amd.LayoutGraph(data['xy'])
    sf.random_seed = 0
    sf.attribute_sign = SIGN[route]
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=api.RADIUS, neighborhood_weighting='triangular')
    sf.load_attributes(attribute_file=data[kind].copy())
    return sf


@pytest.mark.parametrize('route', list(ROUTES))
def test_every_method_scope_and_route(amd, be, data, route):
    keywords, kind, two_sided = ROUTES[route]
    sign = SIGN[route]
    sf = make(amd, data, route)
    ctx = sf._ctx()
    plain = api.run(sf, keywords, multiple_testing=False)
    assert not np.isnan(plain['pvalues_pos']).any()
    num_permutations = keywords.get('num_permutations', 0)
    default = api.run(sf, keywords, multiple_testing=True)             # no keyword: Benjamini-Hochberg on the rows
    assert sf.multiple_testing_method == 'fdr_bh'
    seen = {}
    for method in mt.METHODS:
        for scope in SCOPES:
            got = api.run(sf, keywords, multiple_testing=True, multiple_testing_scope=scope, multiple_testing_method=method)
            assert sf.multiple_testing_method == method and sf.multiple_testing_scope == scope
            q_pos = mt.adjust(plain['pvalues_pos'], scope, method)
            q_neg = mt.adjust(plain['pvalues_neg'], scope, method) if plain['pvalues_neg'] is not None else None
            assert mt.same_bits(got['pvalues_pos'], q_pos), (route, method, scope)
            if q_neg is not None:
                assert mt.same_bits(got['pvalues_neg'], q_neg), (route, method, scope)
            nes, nes_binary, enriched = api.pinned_epilogue(be, ctx, two_sided, q_neg, q_pos, num_permutations, sign)
            assert mt.same_bits(got['nes'], nes), (route, method, scope)
            assert np.array_equal(got['nes_binary'], nes_binary), (route, method, scope)
            assert np.array_equal(got['num_neighborhoods_enriched'], enriched), (route, method, scope)
            seen[method, scope] = got
    sf.multiple_testing_method, sf.multiple_testing_scope = 'fdr_bh', 'attributes'
    for key, value in default.items():               # the default and an explicit 'fdr_bh' are byte-equal to a call without the keyword
        other = seen['fdr_bh', 'attributes'][key]
        assert (value is None and other is None) or mt.same_bits(value, other), key
    # the procedures are told apart on this input.  (Count ratios c / 100 leave the larger families no room -- every non-zero
    # entry of a family of 257 or more becomes 1 under most procedures -- so the rows, families of 70, are asked.)
    rows = {method: fc.bits(seen[method, 'attributes']['pvalues_pos']).tobytes() for method in mt.METHODS}
    assert rows['fdr_bh'] != rows['bonferroni'] and rows['fdr_bh'] != rows['fdr_by'], route


@pytest.mark.parametrize('method', mt.METHODS[1:])
def test_lazy_outputs_on_and_off_agree_and_the_setting_pickles(amd, data, method):
    from safepy_amd.safe import _DeviceResult
    route, scope = 'hypergeom-upper', 'neighborhoods'
    keywords = ROUTES[route][0]
    lazy, eager = make(amd, data, route, lazy=True), make(amd, data, route, lazy=False)
    eager_out = api.run(eager, keywords, multiple_testing=True, multiple_testing_scope=scope, multiple_testing_method=method)
    lazy.compute_pvalues(multiple_testing=True, multiple_testing_scope=scope, multiple_testing_method=method, **keywords)
    assert all(isinstance(lazy.__dict__.get(slot), _DeviceResult) for slot in ('_r_nes', '_r_nes_binary'))
    lazy_out = api.results(lazy)
    for key, value in eager_out.items():
        assert (value is None and lazy_out[key] is None) or mt.same_bits(value, lazy_out[key]), key
    back = pickle.loads(pickle.dumps(lazy))
    assert back.multiple_testing_method == method and back.multiple_testing_scope == scope
    assert mt.same_bits(np.array(back.pvalues_pos, dtype=np.float64), lazy_out['pvalues_pos'])
    assert mt.same_bits(np.array(back.nes_binary, dtype=np.float64), lazy_out['nes_binary'])


def test_refusals_leave_the_results_as_they_were(amd, data):
    route = 'hypergeom-upper'
    keywords = ROUTES[route][0]
    sf = make(amd, data, route)
    before = api.run(sf, keywords, multiple_testing=True, multiple_testing_method='holm')
    for bad in ('sidak', 'holm-sidak', 'BH', 2, None):
        with pytest.raises(ValueError, match='multiple_testing_method'):
            sf.compute_pvalues(multiple_testing=True, multiple_testing_method=bad, **keywords)
        assert sf.multiple_testing_method == 'fdr_bh'
    with pytest.raises(ValueError, match='multiple_testing'):        # two corrections of the same p-values, under every method
        sf.compute_pvalues(how='randomization', num_permutations=100, familywise_adjustment='maxT', multiple_testing=True,
                           multiple_testing_method='hochberg')
    sf.familywise_adjustment = 'none'
    after = api.results(sf)
    for key, value in before.items():
        assert (value is None and after[key] is None) or mt.same_bits(value, after[key]), key


def test_lattice_example(amd):
    """The 18 x 18 lattice with 399 null columns and a planted disc in column 0, analytic normal-tail p-values, every column a
    family: the device's adjusted values against the restatement on the device's own unadjusted p-values, and Holm flags fewer
    null columns at 0.05 than the raw p-values do.  (The table of the documentation comes from a host prototype; its numbers are
    not asserted.)"""
    xy, a, b, planted = mx.planted_lattice()
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy)
    sf.attribute_sign = 'highest'
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='absolute', neighborhood_radius=2.01)
    assert np.array_equal(np.asarray(sf.neighborhoods) != 0, a)
    sf.load_attributes(attribute_file=b.copy())
    keywords = dict(how='analytic')
    plain = api.run(sf, keywords, multiple_testing=False)['pvalues_pos']
    flagged = {'raw': int((plain[:, 1:] <= 0.05).any(axis=0).sum())}
    adjusted = {}
    for method in mt.METHODS:
        got = api.run(sf, keywords, multiple_testing=True, multiple_testing_scope='neighborhoods', multiple_testing_method=method)
        assert mt.same_bits(got['pvalues_pos'], mt.adjust(plain, 'neighborhoods', method)), method
        adjusted[method] = got['pvalues_pos']
        flagged[method] = int((got['pvalues_pos'][:, 1:] <= 0.05).any(axis=0).sum())
    print('null columns flagged at 0.05:', flagged)
    assert flagged['holm'] < flagged['raw']
    assert (adjusted['holm'] != adjusted['hochberg']).sum() > 0
    assert (adjusted['holm'] >= adjusted['hochberg']).all() and (adjusted['bonferroni'] >= adjusted['holm']).all()
    assert (adjusted['fdr_by'] >= adjusted['fdr_bh']).all()
