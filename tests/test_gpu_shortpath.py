"""The bounded all-pairs shortest-path kernel (k_shortpath, K2 in DESIGN.md) on designed graphs, every output against a
reference on the bits: to_dense(), distances() (+inf where a node is not reached), row_counts(), csr(), nnz and
max_row_count.  Needs an MI355X.

The kernel launches W = min(n, 8 * num_cu) one-wave workers; a worker serves the sources worker, worker + W, ... in turn on
the same private scratch (labels, queue flags, two frontier queues, the list of reached nodes) and puts it back by hand
after each search, so every search after a worker's first is right only if that clean-up was complete.  The cases:

  1  n = W + 61 and 2 W + 3 (two and three sources per worker) on shortpath_ref.rung_graph, whose rungs make the sources of
     one worker neighbours: bounded against the oracle, unbounded (every scratch entry of every worker dirtied) against
     SciPy, without the distance matrix, with NULL weights, and every call twice
  2  the workload's own size: the Costanzo surrogate (3971 nodes) through SAFE.define_neighborhoods() with its defaults
  3  frontiers of 63, 64, 65, 128, 129 and 300 entries for the 64 lanes (stars, K(70, 70))
  4  1499 rounds per search (a path of 1500 nodes) against the closed form
  5  labels improved several times within one search (skip graph)
  6  the comparison cand > cutoff: a cutoff exactly at a rounded path sum and one ulp below, 0.0, -1.0, +inf, zero-weight
     cycles and components, -0.0, subnormal weights, self loops, isolated nodes, n = 1, n = 2, no edges, parallel edges
  7  non-finite weights are refused

References are built once per module.  Wall times on the MI355X are in CHANGELOG.md."""
import numpy as np
import pytest

import shortpath_ref as sr
from oracle import safe_oracle as orc            # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


class _Once:
    """References of a module, each built on first use and then shared unchanged."""

    def __init__(self):
        self.memo = {}

    def __call__(self, key, build):
        if key not in self.memo:
            out = build()
            for a in out if isinstance(out, tuple) else (out,):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.memo[key] = out
        return self.memo[key]


@pytest.fixture(scope='module')
def once():
    return _Once()


def _outputs(nbr, distances=True):
    rp, col = nbr.csr()
    out = {'dense': nbr.to_dense(), 'row_counts': nbr.row_counts(), 'row_ptr': rp, 'col': col, 'nnz': nbr.nnz,
           'max_row_count': nbr.max_row_count, 'n': nbr.n}
    if distances:
        out['dist'] = nbr.distances()
    return out


def _run(amd, ctx, g, cutoff, keep_distances=True, weights=True):
    nbr = amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, g.ew if weights else None, cutoff, keep_distances=keep_distances)
    try:
        return _outputs(nbr, distances=keep_distances)
    finally:
        nbr.close()


def _check(got, want_a, want_d, tag=''):
    """Every output of a handle against the reference membership and distances, on the bits."""
    n = want_a.shape[0]
    assert got['n'] == n and got['dense'].dtype == np.int64 and got['dense'].shape == (n, n), tag
    assert np.array_equal(got['dense'], want_a), (tag, 'to_dense', np.argwhere(got['dense'] != want_a)[:5].tolist())
    if 'dist' in got:
        bad = np.argwhere(sr.bits(got['dist']) != sr.bits(want_d))
        assert bad.shape[0] == 0, (tag, 'distances', bad[:5].tolist(), [(got['dist'][i, j], want_d[i, j]) for i, j in bad[:5]])
        assert np.array_equal(got['dist'], want_d), tag
    f = sr.forms(want_a)
    assert np.array_equal(got['row_counts'], f['row_counts']), (tag, 'row_counts')
    assert np.array_equal(got['row_ptr'], f['row_ptr']), (tag, 'csr row_ptr')
    assert np.array_equal(got['col'], f['col']), (tag, 'csr col')
    assert got['nnz'] == f['nnz'] and got['max_row_count'] == f['max_row_count'], (tag, 'info')


def _identical(a, b, tag=''):
    assert a.keys() == b.keys(), tag
    for key in a:
        if key == 'dist':
            assert np.array_equal(sr.bits(a[key]), sr.bits(b[key])), (tag, key)
        else:
            assert np.array_equal(a[key], b[key]), (tag, key)


# --------------------------------------------------------------------- 1. several sources per worker ----

def _rung(ctx, k, weights):
    W = 8 * ctx.num_cu
    g = sr.rung_graph(W, k, weights)
    assert g.n > W, 'n = %d does not pass the %d workers: no worker would serve a second source' % (g.n, W)
    assert g.n == k * W + sr.RUNG_REMAINDER[k] and g.n > k * W
    return g


@pytest.mark.parametrize('weights', ['dyadic', 'real'])
@pytest.mark.parametrize('k', [1, 2])
def test_several_sources_per_worker_bounded(amd, ctx, once, k, weights):
    """n = W + 61 (k = 1: 61 workers serve two sources) and 2 W + 3 (k = 2: three serve three), cutoff 1.0, against the
    oracle; the same call twice gives the same bits (the result does not depend on the order of the atomics)."""
    g = _rung(ctx, k, weights)
    want_a, want_d = once(('rung', k, weights, 1.0), lambda: sr.oracle_reference(g, 1.0))
    first = _run(amd, ctx, g, 1.0)
    _check(first, want_a, want_d, 'first call')
    second = _run(amd, ctx, g, 1.0)
    _check(second, want_a, want_d, 'second call')
    _identical(first, second)


@pytest.mark.parametrize('weights', ['dyadic', 'real'])
def test_several_sources_per_worker_unbounded(amd, ctx, once, weights):
    """n = W + 61, cutoff +inf: every source reaches every node, so every scratch entry of every worker is dirtied and must
    be clean again for the worker's second source.  Against SciPy (positive weights, one edge per pair)."""
    g = _rung(ctx, 1, weights)
    want_a, want_d = once(('rung', 1, weights, np.inf), lambda: sr.scipy_reference(g, np.inf))
    assert want_a.all()                                     # the ring connects everything
    first = _run(amd, ctx, g, np.inf)
    _check(first, want_a, want_d, 'first call')
    second = _run(amd, ctx, g, np.inf)
    _check(second, want_a, want_d, 'second call')
    _identical(first, second)


@pytest.mark.parametrize('weights', ['dyadic', 'real'])
def test_several_sources_per_worker_without_the_distance_matrix(amd, ctx, once, weights):
    """keep_distances=False (dist_out == nullptr in the kernel's epilogue) gives the same membership."""
    g = _rung(ctx, 1, weights)
    want_a, want_d = once(('rung', 1, weights, 1.0), lambda: sr.oracle_reference(g, 1.0))
    nbr = amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, g.ew, 1.0, keep_distances=False)
    try:
        with pytest.raises(amd.SafeHipError):
            nbr.distances()
        _check(_outputs(nbr, distances=False), want_a, want_d)
    finally:
        nbr.close()


def test_several_sources_per_worker_null_weights_are_unit_weights(amd, ctx, once):
    """edge_w=None equals explicit all-ones weights on every output at cutoff 3 (hop counts), and both equal the oracle."""
    g = _rung(ctx, 1, 'ones')
    want_a, want_d = once(('rung', 1, 'ones', 3.0), lambda: sr.oracle_reference(g, 3.0))
    ones = _run(amd, ctx, g, 3.0)
    null = _run(amd, ctx, g, 3.0, weights=False)
    _check(ones, want_a, want_d, 'explicit ones')
    _check(null, want_a, want_d, 'edge_w=None')
    _identical(ones, null)
    _identical(null, _run(amd, ctx, g, 3.0, weights=False), 'edge_w=None twice')


# ------------------------------------------------------------------------ 2. the workload's own size ----

def test_costanzo_surrogate_default_neighborhoods_against_the_oracle(amd, ctx, once):
    """3971 nodes, 28 202 edges, SAFE.define_neighborhoods() with its defaults (shortpath_weighted_layout, 0.1 x the
    layout's x-range): membership and distances against the oracle, not against the kernel's own output."""
    from safepy_amd import workloads
    data = workloads.costanzo_surrogate(seed=0)
    xy, eu, ev, length = data['xy'], data['edge_u'], data['edge_v'], data['length']
    n = xy.shape[0]
    assert n == 3971 and n > 8 * ctx.num_cu, 'n = %d does not pass the %d workers' % (n, 8 * ctx.num_cu)
    cutoff = orc.layout_radius(xy[:, 0], 0.1)
    want_a, want_d = once('costanzo', lambda: orc.neighborhoods_shortpath(n, eu, ev, length, cutoff))
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=length)
    sf.define_neighborhoods()
    assert sf.node_distance_metric == 'shortpath_weighted_layout' and sf.neighborhood_radius == 0.1
    got_a = sf.neighborhoods
    assert got_a.dtype == np.int64 and np.array_equal(got_a, want_a)
    sf.compute_node_distances()
    nd = sf.node_distances
    assert isinstance(nd, dict) and len(nd) == n
    got_d = np.full((n, n), np.inf)
    for s, row in nd.items():
        got_d[s, list(row.keys())] = list(row.values())
    assert np.array_equal(sr.bits(got_d), sr.bits(want_d))
    assert np.array_equal(sf.neighborhoods, want_a)         # compute_node_distances leaves the membership alone


# ------------------------------------------------------------------------------- 3. wide frontiers ----

@pytest.mark.parametrize('cutoff', [1.0, 2.0])
@pytest.mark.parametrize('L', sr.STAR_LEAVES)
def test_wide_frontiers_stars(amd, ctx, once, L, cutoff):
    """K(1, L) with five leaf-to-leaf chords: from the hub a frontier of L entries, from a leaf one of L - 1.  Cutoff 1.0
    keeps every spoke and cuts most two-hop paths; 2.0 keeps every two-hop path (the longest is exactly 2.0)."""
    g = sr.star_graph(L)
    want_a, want_d = once(('star', L, cutoff), lambda: sr.oracle_reference(g, cutoff))
    assert want_a[0].all() and (cutoff < 2.0) == (not want_a.all())
    _check(_run(amd, ctx, g, cutoff), want_a, want_d)


@pytest.mark.parametrize('cutoff', [0.125, 1.0, 2.0, np.inf])
def test_wide_frontiers_complete_bipartite(amd, ctx, once, cutoff):
    """K(70, 70): from 1.0 on the first frontier is a whole side (70 entries), the second the 69 other nodes of the source's
    own side.  0.125 is below every two-hop path but the lightest (1/16 + 1/16), 2.0 above all of them."""
    g = sr.bipartite_graph(70, 70)
    want_a, want_d = once(('bipartite', cutoff), lambda: sr.oracle_reference(g, cutoff))
    assert (cutoff >= 1.0) == bool(want_a.all()) and want_a.sum() > g.n
    _check(_run(amd, ctx, g, cutoff), want_a, want_d)


# --------------------------------------------------------------------------------- 4. deep searches ----

def test_deep_searches_path_of_1500_nodes(amd, ctx):
    """Unbounded on a path: the search from node i runs max(i, 1499 - i) rounds with frontiers of one or two nodes, so the
    queue swap and the two LDS counters are carried through up to 1499 rounds.  Against the exact closed form."""
    g = sr.path_graph(1500)
    want_d = sr.path_closed_form(g)
    _check(_run(amd, ctx, g, np.inf), np.ones((g.n, g.n), dtype=np.int64), want_d)


# ----------------------------------------------------------------------------------- 5. relabelling ----

@pytest.mark.parametrize('cutoff', [np.inf, 8.0])
def test_relabelling_skip_graph(amd, ctx, once, cutoff):
    """513 nodes, edges (i, i + 2^j) of weight 2^j / 16 + j / 64: the coarse hops label a node first and finer paths improve
    it later, so nodes are queued again through their flag within one search.  Cutoff 8.0 drops the hop of 128 (8.109375)
    and two hops of 64 (8.1875), while the unit steps still reach node i + 128 at exactly 8.0."""
    g = sr.skip_graph(513)
    want_a, want_d = once(('skip', cutoff), lambda: sr.oracle_reference(g, cutoff))
    if np.isinf(cutoff):
        assert np.array_equal(sr.bits(want_d), sr.bits(sr.skip_closed_form(513)))
    else:
        assert want_a[0, 128] == 1 and want_d[0, 128] == 8.0 and want_a[0, 129] == 0
    _check(_run(amd, ctx, g, cutoff), want_a, want_d)


# -------------------------------------------------------------- 6. edges of the comparison cand > cutoff ----

EDGE_CASES = [(name, i) for name, (g, cutoffs) in sr.edge_cases().items() for i in range(len(cutoffs))]


@pytest.mark.parametrize('name,i', EDGE_CASES, ids=['%s-%d' % c for c in EDGE_CASES])
def test_edges_of_the_cutoff_comparison(amd, ctx, name, i):
    g, cutoffs = sr.edge_cases()[name]
    cutoff = cutoffs[i]
    want_a, want_d = sr.oracle_reference(g, cutoff)
    got = _run(amd, ctx, g, cutoff)
    _check(got, want_a, want_d, (name, cutoff))
    assert not np.signbit(got['dist']).any()                # 0.0, never -0.0
    if cutoff < 0:
        assert np.array_equal(got['dense'], np.eye(g.n, dtype=np.int64)) and (np.diag(got['dist']) == 0).all()


def test_a_path_exactly_at_the_cutoff_is_kept_and_one_ulp_below_dropped(amd, ctx):
    g = sr.rounding_path()
    at = _run(amd, ctx, g, sr.ROUNDING_CUTOFF)
    below = _run(amd, ctx, g, float(np.nextafter(sr.ROUNDING_CUTOFF, 0)))
    assert at['dense'][0, 3] == 1 and at['dist'][0, 3] == sr.ROUNDING_CUTOFF
    assert below['dense'][0, 3] == 0 and np.isinf(below['dist'][0, 3])
    assert below['dense'][3, 0] == 1 and below['dist'][3, 0] == 0.6     # from its other end the same path sums to 0.6


def test_of_two_edges_between_one_pair_the_lighter_counts(amd, ctx):
    got = _run(amd, ctx, sr.parallel_edges(), np.inf)
    assert got['dist'][0, 1] == 0.25 and got['dist'][1, 2] == 0.5 and got['dist'][2, 3] == 0.125


# ------------------------------------------------------------------------------ 7. infinite weights ----

@pytest.mark.parametrize('bad', [np.inf, np.nan])
@pytest.mark.parametrize('where', [0, -1])
def test_non_finite_weights_are_refused(amd, ctx, bad, where):
    """networkx counts a node behind a path of length +inf as reached when cutoff = +inf; the distance matrix, where +inf
    means unreached, cannot say that, so the entry point refuses the weight like a negative one -- and goes on working."""
    g = sr.rounding_path()
    for cutoff in (np.inf, 1.0):
        ew = g.ew.copy()
        ew[where] = bad
        with pytest.raises(amd.SafeHipError) as err:
            amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, ew, cutoff, keep_distances=True)
        assert err.value.code == -1                         # SAFE_E_INVALID
    ew = g.ew.copy()
    ew[where] = -0.5
    with pytest.raises(amd.SafeHipError) as err:
        amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, ew, 1.0)
    assert err.value.code == -1                             # the same code as a negative weight
    want_a, want_d = sr.oracle_reference(g, 1.0)
    _check(_run(amd, ctx, g, 1.0), want_a, want_d, 'after the refusals')


@pytest.mark.parametrize('u,v', [(3, 0), (0, 3), (-1, 1), (1, -1)])
def test_an_end_point_outside_the_nodes_is_refused(amd, ctx, u, v):
    """the adjacency builder indexes its rows by end point: one outside [0, n) is SAFE_E_INVALID, with and without weights"""
    eu, ev = np.array([0, u], dtype=np.int32), np.array([1, v], dtype=np.int32)
    for ew in (None, np.array([1.0, 1.0])):
        with pytest.raises(amd.SafeHipError) as err:
            amd.Neighborhoods.shortpath(ctx, 3, eu, ev, ew, np.inf, keep_distances=True)
        assert err.value.code == -1                         # SAFE_E_INVALID
