"""SAFE.compute_pvalues(permutation_strata=...): whole calls on the device.  A stratified call must be the call that the table
route makes from the restated tables (tests/strata_ref.py -> backend.Permutations.from_table), bit for bit, on the same
counting kernel as the unstratified call of that shape; it must agree with a NumPy evaluation of those tables by the oracle;
and it must do what the feature is for -- an attribute that is constant inside every stratum has nothing left to test.
Tolerances are the suite's for the same quantities (tests/test_gpu_stream_order.py): observed scores rtol 1e-9 / atol 1e-12,
p-values (count ratios, FDR-adjusted or not) and binarised outputs exact, NES rtol 1e-6 / atol 1e-9.  Needs an MI355X."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (checker only)
import strata_ref as sr                           # noqa: E402

KEY = 0xC0FFEE5AFE
N, P, RADIUS = 300, 50, 0.12
OUTPUTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module', autouse=True)
def nothing_left_for_later_modules():
    """Objects of this module that still own device memory are released when it ends, not by a garbage collection inside a
    later module's busy-stream case (a release waits for the device and would drain that case's stream)."""
    yield
    gc.collect()


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


def make_safe(amd, xy, b, radius=RADIUS, **settings):
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy)
    sf.device_stream_key = KEY
    for name, value in settings.items():
        setattr(sf, name, value)
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=radius)
    sf.load_attributes(attribute_file=b.copy())
    return sf


def results(sf):
    out = {name: np.array(getattr(sf, name)) for name in OUTPUTS}
    out['num_neighborhoods_enriched'] = np.array(sf.attributes['num_neighborhoods_enriched'])
    return out


def same_bytes(got, want, what=''):
    for name in want:
        assert got[name].shape == want[name].shape and got[name].tobytes() == want[name].tobytes(), (what, name)


def through_table(be, sf, table):
    """The same object makes its next call from a caller's table instead of generating one."""
    sf._permutations = lambda ctx, attr, strata: be.Permutations.from_table(ctx, table.astype(np.int32))


def oracle_outputs(a, b, table, score, sign, multiple_testing, threshold=0.05):
    """safe.py:496-554 and 468-472 (oracle.pvalues_by_randomization, binarize) with the permuted matrices b[table[p]]."""
    ns = orc.compute_neighborhood_score(a, b, score)
    cn, cp = np.zeros(ns.shape), np.zeros(ns.shape)
    with np.errstate(invalid='ignore'):
        for row in table:
            sc = orc.compute_neighborhood_score(a, b[row], score)
            cn += sc <= ns
            cp += sc >= ns
    cn[np.isnan(ns)] = np.nan
    cp[np.isnan(ns)] = np.nan
    pn, pp = cn / len(table), cp / len(table)
    if multiple_testing:
        pn, pp = orc.fdr_rows(pn), orc.fdr_rows(pp)
    with np.errstate(invalid='ignore', divide='ignore'):
        nes_pos = -np.log10(np.where(pp == 0, 1 / len(table), pp))
        nes_neg = -np.log10(np.where(pn == 0, 1 / len(table), pn))
    nes = {'highest': nes_pos, 'lowest': nes_neg, 'both': nes_pos - nes_neg}[sign]
    nb, ne = orc.binarize(nes, threshold)
    return {'ns': ns, 'pvalues_neg': pn, 'pvalues_pos': pp, 'nes': nes, 'nes_binary': nb, 'num_neighborhoods_enriched': ne}


def check_against_oracle(got, want):
    np.testing.assert_allclose(got['ns'], want['ns'], rtol=1e-9, atol=1e-12, equal_nan=True)
    for name in ('pvalues_neg', 'pvalues_pos', 'nes_binary', 'num_neighborhoods_enriched'):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    np.testing.assert_allclose(got['nes'], want['nes'], rtol=1e-6, atol=1e-9, equal_nan=True)


# ------------------------------------------------------------------------------------------ the designed confounder ----

@pytest.mark.parametrize('values', ['binary', 'quantitative'])
def test_an_attribute_that_is_its_stratum_has_nothing_to_test(amd, values):
    """60 nodes in a tight cluster far from 240 scattered ones; the attribute marks the cluster and nothing else, and the
    cluster is a stratum.  Freely shuffled, the cluster's neighborhoods (the cluster itself: sum 60 where 12 are expected) are
    enriched.  Shuffled inside the strata the matrix never changes: every permuted score equals the observed one, both counts
    are P, both p-values 1, nes and nes_binary 0 -- exactly."""
    rng = np.random.default_rng(1)
    xy = np.r_[rng.normal(scale=0.003, size=(60, 2)), rng.uniform(1.0, 2.0, size=(240, 2))]
    where = rng.permutation(N)                                               # (the cluster is not the first 60 nodes)
    xy = xy[np.argsort(where)]
    cluster = np.argsort(where) < 60
    hi, lo = (1.0, 0.0) if values == 'binary' else (2.5, -0.75)
    b = np.where(cluster, hi, lo)[:, None] * np.ones((1, 3))
    strata = np.where(cluster, 'cluster', 'elsewhere')

    sf = make_safe(amd, xy, b)
    assert (np.asarray(sf.neighborhoods)[cluster].sum(axis=1) == 60).all()
    sf.compute_pvalues(how='randomization', num_permutations=P)
    free = results(sf)
    assert (free['nes_binary'][cluster] == 1).all() and (free['pvalues_pos'][cluster] == 0).all()
    assert free['num_neighborhoods_enriched'].min() >= 60

    sf.compute_pvalues(how='randomization', num_permutations=P, permutation_strata=strata)
    held = results(sf)
    assert sf.permutation_strata_resolved.tolist() == np.where(cluster, 0, 1).tolist()
    assert sf.permutation_strata_sizes.tolist() == [60, 240]
    np.testing.assert_array_equal(held['ns'], free['ns'])
    for name in ('pvalues_pos', 'pvalues_neg'):
        assert (held[name] == 1).all(), name
    for name in ('nes', 'nes_binary', 'num_neighborhoods_enriched'):
        assert (held[name] == 0).all(), name


# ------------------------------------------------------------------------------------------ bit-equal to the table route ----

def network(n, seed=0):
    return np.random.default_rng(seed).uniform(size=(n, 2))


def attribute_values(kind, n, m, rng):
    if kind == 'binary':
        b = (rng.uniform(size=(n, m)) < 0.15).astype(np.float64)
    else:
        b = np.round(rng.normal(size=(n, m)) * 16) / 16                       # sums of sixteenths are exact: no near-ties
    if kind != 'no_nan':
        b[rng.choice(n, n // 15, replace=False)] = np.nan                     # NaN rows: they never move
        if kind != 'binary':
            b[rng.uniform(size=(n, m)) < 0.02] = np.nan                       # and NaN cells inside rows that do
    return b


# (case, values, settings of the call)
CASES = [
    ('binary', 'binary', {}),
    ('sum', 'quant', {}),
    ('z-score', 'quant', {'neighborhood_score_type': 'z-score'}),
    ('highest', 'quant', {'attribute_sign': 'highest'}),
    ('lowest', 'quant', {'attribute_sign': 'lowest'}),
    ('binary-lowest', 'binary', {'attribute_sign': 'lowest'}),
    ('multiple_testing', 'quant', {'multiple_testing': True}),
    ('rank', 'quant', {'attribute_transform': 'rank'}),
    ('network', 'quant', {'background': 'network'}),
    ('no_nan', 'no_nan', {}),
]


def run_case(amd, be, n, m, values, settings, radius=RADIUS, expect_kernel=None):
    rng = np.random.default_rng(n + m)
    xy = network(n)
    b = attribute_values(values, n, m, rng)
    strata = rng.choice(['a', 'b', 'c', 'd', 'e', 'f', 'g'], size=n, p=[0.4, 0.3, 0.1, 0.1, 0.05, 0.03, 0.02])
    sign = settings.get('attribute_sign', 'both')
    score = settings.get('neighborhood_score_type', 'sum')
    ctx = amd.Context.default(0)

    sf = make_safe(amd, xy, b, radius, attribute_sign=sign)
    call = dict({k: v for k, v in settings.items() if k != 'attribute_sign'}, how='randomization', num_permutations=P)
    sf.compute_pvalues(**call)                                                # the unstratified call of this shape
    kernel = ctx.last_kernel()[0]
    if expect_kernel is not None:
        assert kernel == expect_kernel
    sf = make_safe(amd, xy, b, radius, attribute_sign=sign)
    sf.compute_pvalues(permutation_strata=strata, **call)
    assert ctx.last_kernel()[0] == kernel
    got = results(sf)

    tested = b.copy()                                                         # the matrix the permutation test sees
    if settings.get('background') == 'network':
        tested[np.isnan(tested)] = 0
    if settings.get('attribute_transform') == 'rank':
        from scipy.stats import rankdata
        tested = rankdata(tested, method='average', axis=0, nan_policy='omit')
    movable = (~np.isnan(tested)).any(axis=1)
    ranks = np.unique(strata, return_inverse=True)[1]
    assert np.array_equal(sf.permutation_strata_resolved, ranks) and sf.permutation_strata_resolved.dtype == np.int32
    assert np.array_equal(sf.permutation_strata_sizes, np.bincount(ranks[movable], minlength=7))
    table = sr.strata_tables(n, movable, ranks, P, KEY)

    via = make_safe(amd, xy, b, radius, attribute_sign=sign)
    through_table(be, via, table)
    via.compute_pvalues(permutation_strata=strata, **call)
    same_bytes(got, results(via), 'table route')
    a = np.asarray(sf.neighborhoods).astype(np.float64)
    check_against_oracle(got, oracle_outputs(a, tested, table, score, sign, settings.get('multiple_testing', False)))
    return got


@pytest.mark.parametrize('case,values,settings', CASES, ids=[c[0] for c in CASES])
def test_equals_the_table_route_and_the_oracle(amd, be, case, values, settings):
    run_case(amd, be, N, 9, values, settings)


def test_on_the_blocked_bit_sliced_kernel(amd, be):
    run_case(amd, be, BITS_SHAPE[0], BITS_SHAPE[1], 'binary', {}, radius=BITS_SHAPE[2], expect_kernel='k_permtest_bits_blk')


def test_on_the_matrix_core_kernel(amd, be):
    run_case(amd, be, MFMA_SHAPE[0], MFMA_SHAPE[1], 'quant', {}, radius=MFMA_SHAPE[2], expect_kernel='k_permtest_mfma')


# (nodes, columns, radius) that select the two kernels.  Quantitative blocks of up to 204800 cells stay on the LDS-resident f64
# kernel (enrich.hip, choose_path: `narrow`), so the matrix-core case is the first multiple of ten columns past that at 900 nodes.
BITS_SHAPE = (300, 9, RADIUS)
MFMA_SHAPE = (900, 230, 0.1)


# ------------------------------------------------------------------------------------------------ 'neighborhood_size' ----

@pytest.mark.parametrize('bins', [1, 10, N])
def test_neighborhood_size_strata(amd, be, bins):
    rng = np.random.default_rng(bins)
    xy = np.r_[rng.normal(0.5, 0.08, size=(N // 2, 2)), rng.uniform(size=(N - N // 2, 2))]        # dense middle: sizes vary, with ties
    b = attribute_values('quant', N, 6, rng)
    sf = make_safe(amd, xy, b)
    sf.compute_pvalues(how='randomization', num_permutations=P, permutation_strata='neighborhood_size', permutation_strata_bins=bins)
    got = results(sf)
    sizes = np.asarray(sf.neighborhoods).sum(axis=1)
    want = sr.neighborhood_size_strata(sizes, bins)
    assert len(np.unique(sizes)) < N                                          # ties: cut by node index
    np.testing.assert_array_equal(sf.permutation_strata_resolved, want)
    movable = (~np.isnan(b)).any(axis=1)
    np.testing.assert_array_equal(sf.permutation_strata_sizes, np.bincount(want[movable], minlength=bins))
    via = make_safe(amd, xy, b)
    through_table(be, via, sr.strata_tables(N, movable, want, P, KEY))
    via.compute_pvalues(how='randomization', num_permutations=P, permutation_strata='neighborhood_size', permutation_strata_bins=bins)
    same_bytes(got, results(via))
    if bins == N:                                                             # every stratum one node: nothing moves, p = 1
        ok = ~np.isnan(got['ns'])
        assert (got['pvalues_pos'][ok] == 1).all() and (got['pvalues_neg'][ok] == 1).all() and (got['nes_binary'] == 0).all()
    # the setting (instead of the keyword) does the same, and the INI-style default of 10 bins is what bins=10 gives
    if bins == 10:
        again = make_safe(amd, xy, b, permutation_strata='neighborhood_size')
        again.compute_pvalues(how='randomization', num_permutations=P)
        same_bytes(results(again), got)


# ------------------------------------------------------------------------------------- keys, defaults, memory, refusals ----

def test_seeded_calls_repeat_and_defaults_keep_their_bytes(amd, be):
    rng = np.random.default_rng(3)
    xy = network(N, 3)
    b = attribute_values('quant', N, 5, rng)
    strata = rng.integers(0, 4, size=N)
    movable = (~np.isnan(b)).any(axis=1)

    def run(seed, key=KEY, **kwargs):
        sf = make_safe(amd, xy, b, random_seed=seed)
        sf.device_stream_key = key
        sf.compute_pvalues(how='randomization', num_permutations=P, **kwargs)
        return sf, results(sf)

    _, seeded = run(7, permutation_strata=strata)
    same_bytes(run(7, permutation_strata=strata)[1], seeded, 'a seeded stratified call repeats')
    via = make_safe(amd, xy, b)
    through_table(be, via, sr.strata_tables(N, movable, strata, P, 7))        # the key IS the seed
    via.compute_pvalues(how='randomization', num_permutations=P, permutation_strata=strata)
    same_bytes(results(via), seeded, 'key = random_seed')
    assert run(8, permutation_strata=strata)[1]['pvalues_pos'].tobytes() != seeded['pvalues_pos'].tobytes()
    _, keyed = run(None, permutation_strata=strata)
    same_bytes(run(None, permutation_strata=strata)[1], keyed, 'device_stream_key')
    assert run(None, key=None, permutation_strata=strata)[1]['pvalues_pos'].tobytes() != keyed['pvalues_pos'].tobytes()    # OS entropy
    # the defaults: today's path and bytes, seeded and unseeded
    for seed in (7, None):
        sf, plain = run(seed)
        assert sf.permutation_strata is None and sf.permutation_strata_resolved is None and sf.permutation_strata_sizes is None
        same_bytes(run(seed, permutation_strata=None)[1], plain, 'permutation_strata=None')
    want = orc.compute_pvalues(np.asarray(sf.neighborhoods), b.copy(), enrichment_type='randomization', num_permutations=P, random_seed=7)
    np.testing.assert_array_equal(run(7)[1]['pvalues_pos'], want['pvalues_pos'])


def test_device_memory_is_steady(amd, be):
    rng = np.random.default_rng(4)
    xy = network(N, 4)
    b = attribute_values('quant', N, 5, rng)
    sf = make_safe(amd, xy, b)
    strata = rng.integers(0, 9, size=N)
    live = None
    for call in range(6):
        sf.compute_pvalues(how='randomization', num_permutations=P, permutation_strata=strata)
        if call >= 1:                                 # (the first call grows the context's scratch and parks a handle)
            live = be.device_live_alloc_count() if live is None else live
            assert be.device_live_alloc_count() == live, call


def test_refusals_leave_the_results(amd, be):
    rng = np.random.default_rng(6)
    xy = network(N, 6)
    b = attribute_values('binary', N, 5, rng)
    strata = rng.integers(0, 4, size=N)
    sf = make_safe(amd, xy, b)
    sf.compute_pvalues(how='randomization', num_permutations=P, permutation_strata=strata)
    before = results(sf)
    kept = [getattr(sf, name) for name in OUTPUTS]
    resolved = sf.permutation_strata_resolved
    for kwargs, message in [(dict(how='auto'), "how = 'randomization'"),                     # 0/1 data: the hypergeometric route
                            (dict(how='hypergeometric'), "how = 'randomization'"),
                            (dict(how='analytic'), 'analytic'),
                            (dict(how='randomization', permutation_strata=strata[:-1]), 'expected length'),
                            (dict(how='randomization', permutation_strata=[None] * N), 'missing labels'),
                            (dict(how='randomization', permutation_strata=np.full(N, np.nan)), 'missing labels'),
                            (dict(how='randomization', permutation_strata='degree'), 'not a valid setting'),
                            (dict(how='randomization', permutation_strata_bins=0), 'permutation_strata_bins')]:
        with pytest.raises(ValueError, match=message):
            sf.compute_pvalues(**dict(dict(num_permutations=P, permutation_strata=strata), **kwargs))
        for name, value in zip(OUTPUTS, kept):
            assert getattr(sf, name) is value, (kwargs, name)
        assert sf.permutation_strata_resolved is resolved
        sf.permutation_strata_bins = 10
    same_bytes(results(sf), before)
    # 'neighborhood_size' without neighborhoods
    bare = amd.SAFE(verbose=False)
    bare.node2attribute = b.copy()
    with pytest.raises(ValueError, match='define_neighborhoods'):
        bare.compute_pvalues(how='randomization', permutation_strata='neighborhood_size')
    assert bare.ns is None and bare.pvalues_pos is None


def test_more_than_65535_rows_with_a_value_are_refused(amd, be):
    """The limit of the device generator, met by SAFE before it creates anything: the results of the object stay."""
    n = 65536
    rng = np.random.default_rng(9)
    sf = make_safe(amd, rng.uniform(size=(n, 2)), rng.normal(size=(n, 1)), radius=0.0005)
    marks = {name: object() for name in OUTPUTS}
    for name, mark in marks.items():
        setattr(sf, name, mark)
    with pytest.raises(ValueError, match='65536 rows hold a value'):
        sf.compute_pvalues_by_randomization(num_permutations=10, permutation_strata=np.arange(n) % 3)
    for name, mark in marks.items():
        assert getattr(sf, name) is mark
    assert sf.permutation_strata_resolved is None and sf.permutation_strata_sizes is None
