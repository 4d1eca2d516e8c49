"""SAFE.compute_pvalues with hypergeom_tails = 'attribute_sign' on the device: a 300-node LayoutGraph (the network of
tests/golden/domains.npz), a 70-column 0/1 matrix (its 40 annotations, 28 of them inverted as well so that depletion is as
common as enrichment, one column all zeros, one all ones; some rows all NaN) as dense f64, uint8 and scipy.sparse input; every combination of the
three signs, multiple_testing off / on and lazy_outputs off / on against a host restatement -- SciPy's sf / cdf for the
p-values (rtol 1e-9 where p >= 1e-290), the oracle's Benjamini-Hochberg, tests/hyp_tails_ref.py for NES and nes_binary (cells
within 1e-6 relative of a threshold left out).  The default 'upper' stays what it was, bit for bit.  Needs an MI355X."""
import itertools
import os

import numpy as np
import pytest

import hyp_tails_ref as ht
from oracle import safe_oracle as orc            # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

N, M, RADIUS, THR = 300, 70, 0.2, 0.05
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'domains.npz')
RESULTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


def matrix(with_nan=True):
    g = np.load(GOLDEN)
    base = g['attributes']
    b = np.concatenate([base, 1.0 - base[:, :28], np.zeros((N, 1)), np.ones((N, 1))], axis=1)
    assert b.shape == (N, M) and set(np.unique(b)) == {0.0, 1.0}
    missing = np.zeros(N, dtype=bool)
    if with_nan:
        missing[np.random.default_rng(78).choice(N, 8, replace=False)] = True
        b[missing] = np.nan
    return b, missing


def inputs(kind):
    """(load_attributes kwargs, the dense f64 equivalent)."""
    import scipy.sparse as sp
    if kind == 'dense':
        b, _ = matrix()
        return {'attribute_file': b.copy()}, b
    if kind == 'uint8':                                         # (no missing values in a uint8 matrix)
        b, _ = matrix(with_nan=False)
        return {'attribute_file': b.astype(np.uint8)}, b
    b, missing = matrix()
    return {'attribute_file': sp.csc_array(np.nan_to_num(b)), 'missing_rows': missing.astype(np.uint8)}, b


def new_safe(amd, load, sign, lazy=True):
    g = np.load(GOLDEN)
    xy, eu, ev = g['xy'], g['edge_u'], g['edge_v']
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1)))
    sf.attribute_sign = sign
    sf.lazy_outputs = lazy
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=RADIUS)
    sf.load_attributes(**load)
    return sf


def results(sf):
    out = {key: (None if getattr(sf, key) is None else np.array(getattr(sf, key))) for key in RESULTS}
    out['num_neighborhoods_enriched'] = np.array(sf.attributes['num_neighborhoods_enriched'].values, dtype=np.float64)
    return out


def restatement(a, b, sign, multiple_testing):
    from scipy.stats import hypergeom
    valid = ~np.isnan(b).all(axis=1)
    pop = int(valid.sum())
    K = np.nansum(b, axis=0)
    n = a.astype(np.float64) @ valid.astype(np.float64)
    x = a.astype(np.float64) @ np.nan_to_num(b)
    p_pos = hypergeom.sf(x - 1, pop, K[None, :], n[:, None])
    p_neg = hypergeom.cdf(x, pop, K[None, :], n[:, None])
    if multiple_testing:
        p_pos, p_neg = orc.fdr_rows(p_pos), orc.fdr_rows(p_neg)
    return x, p_pos, p_neg


def near_threshold(p_pos, p_neg, sign):
    """Cells the binarisation is not checked on: the reference p within 1e-6 (relative) of the threshold -- for 'both', the
    ratio p_neg / p_pos within 1e-6 of THR or 1 / THR."""
    with np.errstate(divide='ignore', invalid='ignore'):
        if sign == 'highest':
            return np.abs(p_pos - THR) <= 1e-6 * THR
        if sign == 'lowest':
            return np.abs(p_neg - THR) <= 1e-6 * THR
        ratio = p_neg / p_pos
        return (np.abs(ratio - THR) <= 1e-6 * THR) | (np.abs(ratio - 1 / THR) <= 1e-6 / THR)


@pytest.mark.parametrize('kind', ['dense', 'uint8', 'sparse'])
def test_every_sign_with_and_without_fdr_and_lazy_outputs(amd, kind):
    load, b = inputs(kind)
    a = None
    for sign, mt, lazy in itertools.product(ht.SIGNS, (False, True), (True, False)):
        what = (kind, sign, mt, lazy)
        sf = new_safe(amd, inputs(kind)[0], sign, lazy)
        if a is None:                                           # (the membership mask is pinned to the oracle elsewhere)
            a = np.array(sf.neighborhoods)
        sf.compute_pvalues(hypergeom_tails='attribute_sign', multiple_testing=mt)
        assert sf.hypergeom_tails == 'attribute_sign'
        assert sf._ctx().last_kernel()[0].startswith('k_hyp_tails_emit') or mt, what
        got = results(sf)
        x, p_pos, p_neg = restatement(a, b, sign, mt)
        assert np.array_equal(got['ns'], x), what
        for name, want in (('pvalues_pos', p_pos), ('pvalues_neg', p_neg)):
            big = want >= 1e-290
            np.testing.assert_allclose(got[name][big], want[big], rtol=1e-9, atol=0, err_msg=str(what + (name,)))
            assert (got[name][~big] <= 1.1e-290).all(), what
        nes, nb, counts = ht.outputs(got['pvalues_pos'], got['pvalues_neg'], sign, THR)
        np.testing.assert_allclose(got['nes'], nes, rtol=1e-6, atol=1e-9, err_msg=str(what))
        assert np.array_equal(np.isinf(got['nes']), np.isinf(nes)) and not np.isnan(got['nes']).any(), what
        keep = ~near_threshold(p_pos, p_neg, sign)
        want_nb = ht.outputs(p_pos, p_neg, sign, THR)[1]
        assert np.array_equal(got['nes_binary'][keep], want_nb[keep]), what
        assert np.array_equal(got['num_neighborhoods_enriched'], got['nes_binary'].sum(axis=0)), what
        if sign == 'both':
            assert (got['nes'] < 0).any() and (got['nes'] > 0).any(), what
        if not mt:
            assert got['nes_binary'].sum() > 0, 'the design has no enriched / depleted cell: nothing was tested'


@pytest.mark.parametrize('sign', ht.SIGNS)
def test_default_upper_is_unchanged_whatever_the_sign(amd, sign):
    """hypergeom_tails = 'upper' -- by default, or named -- is the reference's route: the outputs of a call without the kwarg,
    bit for bit, whatever attribute_sign says; pvalues_neg and ns stay unset."""
    load, _ = inputs('dense')
    plain = new_safe(amd, inputs('dense')[0], 'highest')
    plain.compute_pvalues()
    want = results(plain)
    assert want['ns'] is None and want['pvalues_neg'] is None
    assert not plain._ctx().last_kernel()[0].startswith('k_hyp_tails')
    for kwargs in ({}, {'hypergeom_tails': 'upper'}):
        sf = new_safe(amd, inputs('dense')[0], sign)
        sf.compute_pvalues(**kwargs)
        got = results(sf)
        assert sf.hypergeom_tails == 'upper' and got['ns'] is None and got['pvalues_neg'] is None
        for key in ('pvalues_pos', 'nes', 'nes_binary', 'num_neighborhoods_enriched'):
            assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), (sign, kwargs, key)
    with pytest.raises(ValueError, match='hypergeom_tails'):
        sf.compute_pvalues(hypergeom_tails='lower')
    assert sf.hypergeom_tails == 'upper'


def test_downstream_methods_take_the_signed_nes(amd):
    sf = new_safe(amd, inputs('dense')[0], 'both')
    sf.compute_pvalues(hypergeom_tails='attribute_sign')
    pairs = sf.enriched_pairs(values='nes', format='coo', threshold=-np.log10(THR), side='negative')   # compacted on the device
    nes = np.array(sf.nes)
    rows, cols = np.nonzero(nes < -(-np.log10(THR)))
    assert len(rows) > 0, 'the design has no depleted cell: nothing was tested'
    assert np.array_equal(pairs.row, rows) and np.array_equal(pairs.col, cols)
    assert np.array_equal(pairs.data, nes[rows, cols])
    assert (np.array(sf.nes_binary)[rows, cols] == 1).all()
    sf.define_top_attributes()
    sf.define_domains(attribute_distance_threshold=0.75)
    sf.trim_domains()
    assert sf.domains is not None and sf.node2domain is not None


def test_fractional_values_are_refused_before_anything_runs(amd):
    from safepy_amd import backend as be
    b, _ = matrix()
    b[5, 5] = 0.5
    sf = new_safe(amd, {'attribute_file': b}, 'both')
    sf.compute_pvalues(how='hypergeometric')                    # the default route takes such a matrix when forced
    before = {key: getattr(sf, key) for key in RESULTS}
    kernel = sf._ctx().last_kernel()
    live = be.device_live_alloc_count()
    with pytest.raises(ValueError, match='0/1'):
        sf.compute_pvalues(how='hypergeometric', hypergeom_tails='attribute_sign')
    assert sf._ctx().last_kernel() == kernel, 'a kernel ran'
    assert be.device_live_alloc_count() == live
    for key in RESULTS:
        assert getattr(sf, key) is before[key], key
