"""familywise_adjustment = 'maxT' through SAFE.compute_pvalues: seeded calls against the restatement of tests/maxt_ref.py on the
NumPy-stream tables (the stratified ones on tests/strata_ref.py's), bit for bit; the planted lattice; the default; pickling;
refusals that leave the results.  The entry points themselves are pinned in tests/test_gpu_maxt.py.  Needs an MI355X."""
import pickle

import numpy as np
import pytest

from oracle import safe_oracle as orc
import maxt_ref as mx
import strata_ref as sr
import weights_ref as wr

pytestmark = pytest.mark.gpu

RESULTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')
N, M, NPERM, SEED = 150, 12, 30, 5


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
def xy():
    return np.random.default_rng(1).uniform(size=(N, 2))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def values(kind):
    rng = np.random.default_rng(7)
    if kind == 'binary':
        b = (rng.uniform(size=(N, M)) < 0.2).astype(np.float64)
    else:
        b = np.round(rng.normal(size=(N, M)) * 3, 3)
        b[rng.uniform(size=b.shape) < 0.03] = np.nan
    b[rng.choice(N, 10, replace=False)] = np.nan                # nodes without a value
    return b


def make(amd, xy, b, **settings):
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy)
    sf.random_seed = SEED
    weighting = settings.pop('neighborhood_weighting', 'none')
    for key, value in settings.items():
        setattr(sf, key, value)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.15, neighborhood_weighting=weighting)
    sf.load_attributes(attribute_file=b.copy())
    return sf


CASES = [('binary', 'highest', 'neighborhoods', {}),
         ('quantitative', 'lowest', 'all', {'lazy_outputs': False}),
         ('quantitative', 'both', 'neighborhoods', {'attribute_transform': 'rank'}),
         ('quantitative', 'highest', 'all', {'background': 'network'}),
         ('quantitative', 'both', 'neighborhoods', {'permutation_strata': (np.arange(N) % 4).tolist()}),
         ('quantitative', 'highest', 'all', {'neighborhood_weighting': 'triangular'}),
         ('binary', 'both', 'all', {'neighborhood_weighting': 'epanechnikov', 'lazy_outputs': False})]


@pytest.mark.parametrize('kind,sign,scope,extra', CASES, ids=lambda v: v if isinstance(v, str) else '-'.join(sorted(v)) or 'plain')
def test_seeded_call_against_the_restatement(amd, be, ctx, xy, kind, sign, scope, extra):
    from scipy.stats import rankdata
    b = values(kind)
    sf = make(amd, xy, b, attribute_sign=sign, **extra)
    sf.compute_pvalues(how='randomization', num_permutations=NPERM, familywise_adjustment='maxT', familywise_scope=scope)
    assert (sf.familywise_adjustment, sf.familywise_scope) == ('maxT', scope)

    used = b.copy()
    if extra.get('background') == 'network':
        used[np.isnan(used)] = 0
    if extra.get('attribute_transform') == 'rank':
        used = rankdata(used, method='average', axis=0, nan_policy='omit')
    flags = (~np.isnan(used)).any(axis=1)
    a = np.asarray(sf.neighborhoods)
    indptr, indices = wr.csr_of(a)
    w = sf.neighborhood_weights.data.copy() if 'neighborhood_weighting' in extra else None
    if 'permutation_strata' in extra:
        tables = sr.strata_tables(N, flags.astype(np.uint8), np.asarray(extra['permutation_strata']), NPERM, SEED)
    else:
        tables = orc.permutation_index_table(used, NPERM, SEED)
    attr = be.Attributes.from_host(ctx, used)
    try:
        mu, q = attr.column_moments()                          # (the contract takes them from safe_attr_column_moments)
    finally:
        attr.close()
    loc, scale = mx.row_factors(indptr, indices, flags, int(flags.sum()), w)
    z, live, tmax, tmin, _ = mx.extremes(indptr, indices, w, used, tables, loc, scale, mu, q)
    neg, pos, least_neg, least_pos = mx.counts(z, live, tmax, tmin, mx.MATRIX if scope == 'all' else mx.COLUMN)
    want = {'ns': wr.score(indptr, indices, np.ones(len(indices)) if w is None else w, used),
            'pvalues_neg': neg / NPERM, 'pvalues_pos': pos / NPERM}
    with np.errstate(divide='ignore'):
        nes_pos = -np.log10(np.where(want['pvalues_pos'] == 0, 1 / NPERM, want['pvalues_pos']))
        nes_neg = -np.log10(np.where(want['pvalues_neg'] == 0, 1 / NPERM, want['pvalues_neg']))
    want['nes'] = {'highest': nes_pos, 'lowest': nes_neg, 'both': nes_pos - nes_neg}[sign]
    want['nes_binary'], enriched = orc.binarize(want['nes'], sf.enrichment_threshold)
    for name in RESULTS:
        assert np.array_equal(bits(getattr(sf, name)), bits(want[name])), name
    assert np.array_equal(bits(sf.familywise_statistic), bits(z)), 'familywise_statistic'
    assert np.array_equal(sf.attributes['num_neighborhoods_enriched'].to_numpy(), enriched)
    assert np.array_equal(sf.attributes['familywise_pvalue_pos'].to_numpy(), least_pos / NPERM)
    assert np.array_equal(sf.attributes['familywise_pvalue_neg'].to_numpy(), least_neg / NPERM)
    assert np.array_equal(sf.attributes['familywise_pvalue_pos'].to_numpy(),
                          np.where(live, want['pvalues_pos'], 1.0).min(axis=0))


def test_planted_lattice(amd):
    """18 x 18 lattice, 13-member discs, 40 standard-normal columns with +1.5 planted on a radius-3 disc of column 0, P = 200:
    the adjusted calls are a subset of the unadjusted ones, and the planted attribute is found at the attribute level."""
    xy, a, b, planted = mx.planted_lattice(m=40)
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy)
    sf.random_seed = 3
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius_type='absolute', neighborhood_radius=2.01)
    assert np.array_equal(np.asarray(sf.neighborhoods) != 0, a)
    sf.load_attributes(attribute_file=b.copy())
    sf.compute_pvalues(how='randomization', num_permutations=200)
    plain = np.array(sf.nes_binary)
    plain_p = np.array(sf.pvalues_pos)
    sf.compute_pvalues(how='randomization', num_permutations=200, familywise_adjustment='maxT')
    adjusted = np.array(sf.nes_binary)
    assert (adjusted <= plain).all() and adjusted.sum() < plain.sum()
    assert (np.array(sf.pvalues_pos) >= plain_p).all()
    assert sf.attributes['familywise_pvalue_pos'][0] <= 0.05
    assert adjusted[planted, 0].sum() >= 1
    null_hits = int(np.count_nonzero(sf.attributes['familywise_pvalue_pos'].to_numpy()[1:] <= 0.05))
    print('null columns flagged after the adjustment: %d of 39 (before: %d)' % (null_hits, int((plain[:, 1:].sum(axis=0) > 0).sum())))
    assert null_hits <= 8          # 0.05 * 39 + 5 sigma = 8.76, sigma = sqrt(39 * 0.05 * 0.95) = 1.36


def test_default_pickle_and_refusals(amd, xy):
    b = values('quantitative')
    sf = make(amd, xy, b)
    sf.compute_pvalues(how='randomization', num_permutations=NPERM)
    plain = {name: np.array(getattr(sf, name)) for name in RESULTS}
    assert sf.familywise_statistic is None and 'familywise_pvalue_pos' not in sf.attributes
    other = make(amd, xy, b)
    other.compute_pvalues(how='randomization', num_permutations=NPERM, familywise_adjustment='none')
    for name in RESULTS:
        assert np.array_equal(bits(getattr(other, name)), bits(plain[name])), 'the default: ' + name

    other.compute_pvalues(how='randomization', num_permutations=NPERM, familywise_adjustment='maxT', familywise_scope='all')
    back = pickle.loads(pickle.dumps(other))
    assert (back.familywise_adjustment, back.familywise_scope) == ('maxT', 'all')
    for name in RESULTS + ('familywise_statistic',):
        assert np.array_equal(bits(getattr(back, name)), bits(getattr(other, name))), name
    assert np.array_equal(back.attributes['familywise_pvalue_pos'].to_numpy(), other.attributes['familywise_pvalue_pos'].to_numpy())
    back.compute_pvalues(how='randomization', num_permutations=NPERM)            # the loaded settings: the same call again
    for name in RESULTS + ('familywise_statistic',):
        assert np.array_equal(bits(getattr(back, name)), bits(getattr(other, name))), 'after loading: ' + name

    kept = {name: getattr(other, name) for name in RESULTS + ('familywise_statistic',)}
    binary = make(amd, xy, values('binary'))
    for target, kwargs, message in [(other, dict(how='analytic'), "how = 'randomization'"),
                                    (other, dict(how='hypergeometric'), "how = 'randomization'"),
                                    (other, dict(how='randomization', neighborhood_score_type='z-score'), 'z-score'),
                                    (other, dict(how='randomization', multiple_testing=True), 'multiple_testing'),
                                    (binary, dict(how='auto', familywise_adjustment='maxT'), "how = 'randomization'")]:
        with pytest.raises(ValueError, match=message):
            target.compute_pvalues(**kwargs)
        target.neighborhood_score_type, target.multiple_testing = 'sum', False
    for name, value in kept.items():
        assert getattr(other, name) is value, name
    assert binary.ns is None and binary.nes is None and binary.familywise_statistic is None
