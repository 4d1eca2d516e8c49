"""The graphs and references of tests/shortpath_ref.py without a device: the two references against each other wherever
SciPy is allowed, every closed form against the oracle, and the size rule that makes rung_graph() put two or three sources
on one worker of the shortest-path kernel."""
import numpy as np
import pytest

import shortpath_ref as sr

W_SMALL = 40                                # stands for 8 * num_cu: n = 101 and 83


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(sr.bits(got[1]), sr.bits(want[1]))


def _builders():
    """Every builder at a reduced size, with the cutoffs its GPU test uses."""
    inf = np.inf
    out = []
    for k in (1, 2):
        for weights in ('dyadic', 'real'):
            out.append(('rung k=%d %s' % (k, weights), sr.rung_graph(W_SMALL, k, weights), [1.0, inf]))
        out.append(('rung k=%d ones' % k, sr.rung_graph(W_SMALL, k, 'ones'), [3.0]))
    for L in (5, 63, 65):
        out.append(('star %d' % L, sr.star_graph(L), [1.0, 2.0]))
    out.append(('bipartite', sr.bipartite_graph(9, 11), [0.125, 1.0, 2.0, inf]))
    out.append(('path', sr.path_graph(150), [inf, 3.0]))
    out.append(('skip', sr.skip_graph(65), [inf, 1.0]))
    for name, (g, cutoffs) in sr.edge_cases().items():
        out.append((name, g, cutoffs))
    return out


BUILDERS = _builders()


@pytest.mark.parametrize('name,g,cutoffs', BUILDERS, ids=[b[0] for b in BUILDERS])
def test_scipy_and_the_oracle_agree_wherever_scipy_is_allowed(name, g, cutoffs):
    assert g.eu.shape == g.ev.shape == g.ew.shape and g.eu.dtype == np.int32 and g.ew.dtype == np.float64
    assert g.eu.size == 0 or (0 <= min(g.eu.min(), g.ev.min()) and max(g.eu.max(), g.ev.max()) < g.n)
    for cutoff in cutoffs:
        want = sr.oracle_reference(g, cutoff)
        assert np.array_equal(want[0], np.isfinite(want[1]))                    # +inf is "unreached" and nothing else
        assert not np.signbit(want[1]).any()                                    # no -0.0
        assert np.array_equal(np.diag(want[1]), np.zeros(g.n))
        if sr.scipy_allowed(g) and cutoff >= 0:
            assert _same(sr.scipy_reference(g, cutoff), want), (name, cutoff)


def test_scipy_is_allowed_where_expected():
    allowed = {name for name, g, _ in BUILDERS if sr.scipy_allowed(g)}
    assert {'rung k=1 dyadic', 'rung k=2 real', 'rung k=1 ones', 'star 63', 'bipartite', 'path', 'skip', 'rounding_path',
            'subnormal', 'no_edges'} <= allowed
    assert not allowed & {'zero_mix', 'zero_components', 'negative_zero', 'parallel_edges', 'loops_and_isolated'}
    with pytest.raises(AssertionError):
        sr.scipy_reference(sr.parallel_edges(), 1.0)


@pytest.mark.parametrize('weights', ['dyadic', 'real', 'ones'])
@pytest.mark.parametrize('W', [2, 7, W_SMALL, 61, 2048])
@pytest.mark.parametrize('k', [1, 2])
def test_rung_graph_size_rule(W, k, weights):
    g = sr.rung_graph(W, k, weights)
    r = {1: 61, 2: 3}[k]
    assert g.n == k * W + r and g.n > k * W                 # some worker of W serves k + 1 sources
    pairs = set(zip(np.minimum(g.eu, g.ev).tolist(), np.maximum(g.eu, g.ev).tolist()))
    assert len(pairs) == g.eu.shape[0]                      # one edge per pair
    assert all(a != b for a, b in pairs)
    for i in range(g.n - W):
        assert (i, i + W) in pairs                          # the sources of one worker are adjacent
    for i in range(g.n):
        assert (min(i, (i + 1) % g.n), max(i, (i + 1) % g.n)) in pairs
    assert 2 * g.n - W <= len(pairs) <= 2 * g.n - W + g.n // 2         # ring and rungs are distinct pairs; then the chords
    if g.n >= 80:
        assert len(pairs) > 2 * g.n - W + g.n // 4                      # most of the n / 2 chords survive
    if weights == 'dyadic':
        assert np.array_equal(g.ew * 16, np.round(g.ew * 16)) and g.ew.min() >= 1 / 16 and g.ew.max() <= 1.0
    elif weights == 'real':
        assert g.ew.min() >= 0.01 and g.ew.max() < 1.0
    else:
        assert np.array_equal(g.ew, np.ones(g.eu.shape[0]))
    assert sr.scipy_allowed(g)


def test_rung_graph_later_sources_meet_earlier_labels_from_both_sides():
    """What the rungs are for: of the nodes both searches of one worker label, some are nearer to the later source and some
    farther, so a label left behind is wrong in both directions."""
    g = sr.rung_graph(W_SMALL, 1, 'dyadic')
    d = sr.oracle_reference(g, 1.0)[1]
    nearer = farther = 0
    for s in range(g.n - W_SMALL):
        both = np.isfinite(d[s]) & np.isfinite(d[s + W_SMALL])
        nearer += int((d[s + W_SMALL][both] < d[s][both]).sum())
        farther += int((d[s + W_SMALL][both] > d[s][both]).sum())
    assert nearer > 100 and farther > 100


def test_path_closed_form():
    g = sr.path_graph(150)
    want = sr.path_closed_form(g)
    assert np.array_equal(sr.bits(sr.oracle_reference(g, np.inf)[1]), sr.bits(want))
    g = sr.path_graph()                                     # the size the GPU test runs, against the fast reference
    assert g.n == 1500
    want = sr.path_closed_form(g)
    assert np.array_equal(want * 16, np.round(want * 16)) and want.max() < 2.0 ** 40
    assert np.array_equal(sr.bits(sr.scipy_reference(g, np.inf)[1]), sr.bits(want))


def test_skip_closed_form_and_coarse_hops_label_first():
    g = sr.skip_graph(65)
    assert np.array_equal(sr.bits(sr.oracle_reference(g, np.inf)[1]), sr.bits(sr.skip_closed_form(65)))
    g = sr.skip_graph()
    assert g.n == 513 and g.eu.shape[0] == sum(513 - (1 << j) for j in range(10))
    assert np.array_equal(sr.bits(sr.scipy_reference(g, np.inf)[1]), sr.bits(sr.skip_closed_form(513)))
    span = (g.ev - g.eu).astype(np.float64)
    assert (g.ew[span > 1] > span[span > 1] / 16).all()     # every coarse hop is longer than the unit steps under it


def test_star_closed_form_and_frontier_sizes():
    assert sr.STAR_LEAVES == (63, 64, 65, 128, 129, 300)
    for L in (63, 65):
        g = sr.star_graph(L, chords=0)
        assert g.n == L + 1 and g.eu.shape[0] == L
        assert np.array_equal(sr.bits(sr.oracle_reference(g, np.inf)[1]), sr.bits(sr.star_closed_form(g)))
    g = sr.star_graph(300)
    assert g.eu.shape[0] == 305 and (g.eu[:300] == 0).all() and (g.eu[300:] > 0).all()
    assert g.ew.max() <= 1.0                                # cutoff 1.0: the hub's first frontier is every leaf
    assert np.isfinite(sr.oracle_reference(g, 1.0)[1][0]).all()


def test_zero_components_closed_form():
    g = sr.zero_components()
    a, d = sr.oracle_reference(g, np.inf)
    comp = np.array([0] * 7 + [1] * 5 + [2] * 2 + [3])
    assert np.array_equal(a, (comp[:, None] == comp[None, :]).astype(np.int64))
    assert np.array_equal(sr.bits(d[a == 1]), np.zeros(int(a.sum()), dtype=np.uint64))     # 0.0, never -0.0
    assert np.array_equal(sr.oracle_reference(g, 0.0)[0], a) and np.array_equal(sr.oracle_reference(g, -1.0)[0], np.eye(15))


def test_designed_edges_of_the_cutoff_comparison():
    g = sr.rounding_path()
    assert sr.ROUNDING_CUTOFF == 0.6000000000000001 and (0.3 + 0.2) + 0.1 == 0.6
    at, below = sr.oracle_reference(g, sr.ROUNDING_CUTOFF), sr.oracle_reference(g, np.nextafter(sr.ROUNDING_CUTOFF, 0))
    assert at[0][0, 3] == 1 and at[1][0, 3] == sr.ROUNDING_CUTOFF and below[0][0, 3] == 0
    assert below[0][3, 0] == 1 and below[1][3, 0] == 0.6    # the same path from its other end rounds differently
    g = sr.subnormal()
    at, below = sr.oracle_reference(g, sr.SUBNORMAL_CUTOFF), sr.oracle_reference(g, np.nextafter(sr.SUBNORMAL_CUTOFF, 0))
    assert 0 < sr.SUBNORMAL_CUTOFF < 2.3e-308 and at[0][0, 3] == 1 and at[0][0, 4] == 0 and below[0][0, 3] == 0
    g = sr.parallel_edges()
    d = sr.oracle_reference(g, np.inf)[1]
    assert d[0, 1] == 0.25 and d[1, 2] == 0.5 and d[2, 3] == 0.125          # the lighter of the two, wherever it stands
    g = sr.negative_zero()
    assert np.signbit(g.ew).sum() == 3
    g = sr.zero_mix()
    a = sr.oracle_reference(g, 0.0)[0]
    assert a[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0] and a[5].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 0, 0]
    for name, (g, cutoffs) in sr.edge_cases().items():
        assert g.n <= 40, name


def test_forms():
    a = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 1]])
    f = sr.forms(a)
    assert f['row_counts'].tolist() == [2, 0, 3] and f['row_ptr'].tolist() == [0, 2, 2, 5]
    assert f['col'].tolist() == [0, 2, 0, 1, 2] and f['nnz'] == 5 and f['max_row_count'] == 3
    assert f['row_ptr'].dtype == np.int32 and f['col'].dtype == np.int32
