"""The Kamada-Kawai layout on the device (kk.hip, safe_kk_*): the cost function against tests/kk_ref.py -- networkx's
_kamada_kawai_costfn restated, held to the real function by tests/test_kk_ref_cpu.py -- on the bits of cost and gradient,
and safe_io.kamada_kawai_layout against nx.kamada_kawai_layout's recorded positions (tests/golden/kk.npz) on the bits of
the coordinates."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kk_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kk.npz')
ROWS, CHUNK = 16, 64            # kk.hip: rows per workgroup, columns per chunk
# kk_ref.SIZES, two sizes whose chains span many chunks, and the kernel's own tile edges
SIZES = tuple(sorted(set(kk_ref.SIZES + (1025, 2049, ROWS - 1, ROWS, ROWS + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1))))


def _ctx():
    from safepy_amd import backend as be
    return be.Context.default(0)


@functools.lru_cache(maxsize=None)
def _case(n, weighted):
    """(host distance matrix as the device computed it, inf where unreached; handle from it; handle from the membership)."""
    from safepy_amd import backend as be
    eu, ev, ew = kk_ref.sparse_edges(n, seed=400 + n, weighted=weighted)
    nbr = be.Neighborhoods.shortpath(_ctx(), n, eu, ev, ew, np.inf, keep_distances=True)
    dist = nbr.distances()
    from_nbr = be.KamadaKawai.from_neighborhoods(_ctx(), nbr)
    nbr.close()
    return dist, be.KamadaKawai.from_distances(_ctx(), dist), from_nbr


def _dist_mtx(dist):
    return np.where(np.isinf(dist), kk_ref.UNREACHED, dist)


def _compare(tag, got, want):
    (cost, grad), (want_cost, want_grad) = got, want
    assert kk_ref.same_bits([cost], [want_cost]), (tag, 'cost', float(cost), float(want_cost))
    bad = np.flatnonzero(~((kk_ref.bits(grad) == kk_ref.bits(want_grad)) | (np.isnan(grad) & np.isnan(want_grad))))
    assert bad.size == 0, (tag, 'gradient entries', bad[:8], grad[bad[:8]], want_grad[bad[:8]])


@pytest.mark.parametrize('n', SIZES)
def test_cost_and_gradient_equal_the_restatement_bit_for_bit(n):
    import scipy.optimize
    weighted = n % 2 == 1 or n >= 128           # both kinds at every regime of sizes; the large ones weighted
    dist, from_host, from_nbr = _case(n, weighted)
    if n >= 3:
        assert np.isinf(dist).any()             # a disconnected part: 1e6 entries
    invdist = kk_ref.invdist_of(_dist_mtx(dist))
    stepped = scipy.optimize.minimize(from_host.evaluate, kk_ref.positions(n, 'circle').ravel(), method='L-BFGS-B', jac=True,
                                      options={'maxiter': 3}).x
    for kind, pos in (('random', kk_ref.positions(n, 'random', seed=n)), ('circle', kk_ref.positions(n, 'circle')),
                      ('stepped', stepped)):
        want = kk_ref.kk_costfn_ref(pos.ravel(), invdist)
        a, b = from_host.evaluate(pos), from_nbr.evaluate(pos)
        _compare((n, kind, 'host matrix'), a, want)
        assert kk_ref.same_bits([a[0]], [b[0]]) and kk_ref.same_bits(a[1], b[1]), (n, kind, 'host matrix vs membership handle')


def test_unweighted_distances_of_the_device_are_networkx_dist_mtx():
    """The matrix the membership handle hands over is kamada_kawai_layout's dist_mtx (1e6 for inf), weighted too."""
    for n, weighted in ((91, False), (129, True)):
        eu, ev, ew = kk_ref.sparse_edges(n, seed=400 + n, weighted=weighted)
        want = kk_ref.nx_dist_mtx(kk_ref.nx_graph(n, eu, ev, ew))
        assert np.array_equal(kk_ref.bits(_dist_mtx(_case(n, weighted)[0])), kk_ref.bits(want))


def test_a_distance_matrix_asymmetric_in_the_last_bit_is_read_entry_by_entry():
    from safepy_amd import backend as be
    n = 130
    dist = _dist_mtx(_case(n, True)[0]).copy()
    rng = np.random.default_rng(3)
    for _ in range(12):
        i, j = rng.integers(0, n, size=2)
        if i != j:
            dist[i, j] = np.nextafter(dist[i, j], np.inf)
    assert not np.array_equal(dist, dist.T)
    kk = be.KamadaKawai.from_distances(_ctx(), dist)
    pos = kk_ref.positions(n, 'random', seed=9)
    _compare('asymmetric', kk.evaluate(pos), kk_ref.kk_costfn_ref(pos.ravel(), kk_ref.invdist_of(dist)))
    kk.close()


def test_coincident_nodes_put_nan_where_networkx_does():
    n = 91
    dist, kk, _ = _case(n, True)
    pos = kk_ref.positions(n, 'random', seed=2)
    pos[4] = pos[2]
    pos[70] = pos[2]
    want = kk_ref.kk_costfn_ref(pos.ravel(), kk_ref.invdist_of(_dist_mtx(dist)))
    nan = np.isnan(want[1])
    assert nan.any() and not nan.all()
    got = kk.evaluate(pos)
    assert np.array_equal(np.isnan(got[1]), nan)
    _compare('coincident', got, want)


def test_evaluating_twice_gives_identical_bits():
    n = 513
    _, kk, _ = _case(n, True)
    pos = kk_ref.positions(n, 'random', seed=4)
    a, b = kk.evaluate(pos), kk.evaluate(pos.copy())
    assert np.array_equal(kk_ref.bits([a[0]]), kk_ref.bits([b[0]])) and np.array_equal(kk_ref.bits(a[1]), kk_ref.bits(b[1]))


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


CASES = ('gnp1', 'gnp2', 'gnp3', 'gnp50', 'gnp130', 'gnp300', 'gnp600', 'weighted', 'twocomp')


@pytest.mark.parametrize('case', CASES)
def test_layout_of_a_networkx_graph_equals_networkx_bit_for_bit(case):
    from safepy_amd import safe_io
    g = _golden()
    n = int(g[case + '_n'])
    G = kk_ref.nx_graph(n, g[case + '_u'], g[case + '_v'], g.get(case + '_w'))
    pos = safe_io.kamada_kawai_layout(G)
    assert list(pos) == list(range(n))
    got = np.array([pos[i] for i in range(n)]).reshape(n, 2)
    assert np.array_equal(kk_ref.bits(got), kk_ref.bits(g[case + '_pos'])), np.abs(got - g[case + '_pos']).max()


@pytest.mark.parametrize('case', CASES)
def test_layout_of_a_layout_graph_equals_networkx_bit_for_bit(case):
    import safepy_amd
    from safepy_amd import safe_io
    g = _golden()
    n = int(g[case + '_n'])
    G = safepy_amd.LayoutGraph(np.zeros((n, 2)), g[case + '_u'], g[case + '_v'], weight=g.get(case + '_w'))
    assert safe_io.kamada_kawai_layout(G) is G
    assert np.array_equal(kk_ref.bits(G.xy), kk_ref.bits(g[case + '_pos']))


def test_scale_center_and_a_given_start_follow_networkx():
    import networkx as nx
    from safepy_amd import safe_io
    g = _golden()
    n = int(g['gnp50_n'])
    G = kk_ref.nx_graph(n, g['gnp50_u'], g['gnp50_v'])
    start = {i: p for i, p in enumerate(kk_ref.positions(n, 'random', seed=8))}
    dist = dict(nx.shortest_path_length(G))
    with np.errstate(all='ignore'):
        want = nx.kamada_kawai_layout(G, dist=dist, pos=start, scale=3, center=(1.5, -2))
    got = safe_io.kamada_kawai_layout(G, dist=dist, pos=start, scale=3, center=(1.5, -2))
    assert all(np.array_equal(kk_ref.bits(got[i]), kk_ref.bits(want[i])) for i in range(n))


def test_load_network_from_txt_with_the_kamada_kawai_layout(tmp_path):
    from safepy_amd import safe_io
    g = _golden()
    labels = g['txt_labels']
    path = tmp_path / 'net.txt'
    path.write_text(''.join('L%d\tL%d\t1\n' % (labels[u], labels[v]) for u, v in zip(g['txt_u'], g['txt_v'])))
    G = safe_io.load_network_from_txt(str(path), layout='kamada_kawai', verbose=False)
    n = int(g['txt_n'])
    assert [G.nodes[i]['label'] for i in range(n)] == ['L%d' % k for k in labels]
    xy = np.array([[G.nodes[i]['x'], G.nodes[i]['y']] for i in range(n)])
    assert np.array_equal(kk_ref.bits(xy), kk_ref.bits(g['txt_pos']))
    length = np.array([G[int(u)][int(v)]['length'] for u, v in zip(g['txt_u'], g['txt_v'])])
    assert np.array_equal(kk_ref.bits(length), kk_ref.bits(g['txt_length']))


def test_safe_load_network_passes_the_layout_on(tmp_path):
    import safepy_amd
    g = _golden()
    labels = g['txt_labels']
    path = tmp_path / 'net.txt'
    path.write_text(''.join('L%d\tL%d\t1\n' % (labels[u], labels[v]) for u, v in zip(g['txt_u'], g['txt_v'])))
    sf = safepy_amd.SAFE(verbose=False)
    sf.load_network(network_file=str(path), layout='kamada_kawai', node_key_attribute='key')
    n = int(g['txt_n'])
    xy = np.array([[sf.graph.nodes[i]['x'], sf.graph.nodes[i]['y']] for i in range(n)])
    assert np.array_equal(kk_ref.bits(xy), kk_ref.bits(g['txt_pos']))


def test_refusals():
    from safepy_amd import _lib, backend as be
    ctx = _ctx()
    small = np.zeros((2, 2))
    h = C.c_void_p()
    # above the stated limit: refused from n alone, before the matrix is read
    assert _lib.lib.safe_kk_create_host(ctx.handle, C.c_void_p(small.ctypes.data), _lib.KK_MAX_NODES + 1, C.byref(h)) == _lib.E_UNSUPPORTED
    assert not h.value
    for bad in (np.nan, -1.0):
        d = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, bad], [2.0, 1.0, 0.0]])
        with pytest.raises(be._lib.SafeHipError) as err:
            be.KamadaKawai.from_distances(ctx, d)
        assert err.value.code == _lib.E_VALUE
    nbr = be.Neighborhoods.shortpath(ctx, 3, [0], [1], None, np.inf, keep_distances=False)
    with pytest.raises(be._lib.SafeHipError) as err:
        be.KamadaKawai.from_neighborhoods(ctx, nbr)
    assert err.value.code == _lib.E_INVALID
    nbr.close()
    kk = be.KamadaKawai.from_distances(ctx, np.array([[0.0, 1.0], [1.0, 0.0]]))
    with pytest.raises(ValueError):
        kk.evaluate(np.zeros(3))
    kk.close()
