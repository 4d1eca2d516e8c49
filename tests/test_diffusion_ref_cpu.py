"""node_distance_metric = 'diffusion' without a device: the NumPy restatement of the contract (tests/diffusion_ref.py) against exact
rationals, the resolvent and a closed form; the properties that make the distance useful; the settings, INI keys and pickling; the
refusals that need no device; the new symbols in header, binding and library.

The iteration X_{t+1} = alpha I + beta S X_t from X_0 = I gives, in exact arithmetic,
    X_T = alpha sum_{t < T} (beta S)^t + (beta S)^T,
the restart-weighted series whose last term has full weight (X_0 = I, not alpha I).  The closed forms below use this."""
import configparser
import ctypes
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest

import diffusion_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                    # unit roundoff of f64


def rounding_bound(max_entries, steps):
    """First-order relative error bound of an element of the f64 run, doubled for the higher orders.  Every term of every sum is
    >= 0, so nothing cancels and relative errors add: an entry s_ik carries 4 roundings (r_i, r_k, two products); an element of a
    step the product's, one per add of the row, beta's product and alpha's add: (4 + 1 + max_entries + 2) u per step."""
    return 2.0 * (7 + max_entries) * steps * U


# ------------------------------------------------------------------------------------------------ exact rationals ----

# The hand-made graph: every weighted degree is a perfect square, so r_i and s_ik are rational.
#   edges (u, v, w): 0-1 1 | 0-1 2 (a duplicate) | 0-2 1 | 1-2 3 | 1-4 3 | 2-2 5 (a self-loop: one entry) | 3-4 1
#   d = 4, 9, 9, 1, 4      r = 1/2, 1/3, 1/3, 1, 1/2
HAND = (np.array([0, 0, 0, 1, 1, 2, 3]), np.array([1, 1, 2, 2, 4, 2, 4]), np.array([1.0, 2.0, 1.0, 3.0, 3.0, 5.0, 1.0]))
HAND_R = [Fraction(1, 2), Fraction(1, 3), Fraction(1, 3), Fraction(1), Fraction(1, 2)]


def hand_exact(alpha, steps):
    eu, ev, w = HAND
    n = 5
    s = [[Fraction(0)] * n for _ in range(n)]
    for u, v, x in zip(eu.tolist(), ev.tolist(), w.tolist()):
        s[u][v] += Fraction(x) * HAND_R[u] * HAND_R[v]
        if u != v:
            s[v][u] += Fraction(x) * HAND_R[u] * HAND_R[v]
    beta = 1 - alpha
    x = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for _ in range(steps):
        x = [[(alpha if i == j else 0) + beta * sum(s[i][k] * x[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    return s, x


def test_csr_order_and_degrees_of_the_hand_graph():
    ptr, col, w = dr.csr(5, *HAND)
    assert ptr.tolist() == [0, 3, 7, 10, 11, 13]
    assert col.tolist() == [1, 1, 2, 0, 0, 2, 4, 0, 1, 2, 4, 1, 3]
    assert w.tolist() == [1, 2, 1, 1, 2, 3, 3, 1, 3, 5, 1, 3, 1]      # duplicates in input order, the self-loop once
    r, _ = dr.scaled(ptr, col, w)
    assert r.tolist() == [0.5, 1 / 3, 1 / 3, 1.0, 0.5]


@pytest.mark.parametrize('alpha,steps', [(Fraction(1, 2), 1), (Fraction(1, 2), 3), (Fraction(1, 10), 3), (Fraction(9, 10), 2)])
def test_kernel_against_exact_rationals(alpha, steps):
    s, want = hand_exact(alpha, steps)
    # by hand: the duplicate edges add, s_01 = 1/6 + 1/3; the self-loop is s_22 = 5/9; one step from X_0 = I is alpha I + beta S
    assert s[0][1] == Fraction(1, 2) and s[2][2] == Fraction(5, 9) and s[3][4] == Fraction(1, 2) and s[0][3] == 0
    if steps == 1 and alpha == Fraction(1, 2):
        assert want[0][1] == Fraction(1, 4) and want[2][2] == Fraction(1, 2) + Fraction(5, 18) and want[0][4] == 0
    got = dr.kernel(5, *HAND, float(alpha), steps)
    bound = rounding_bound(4, steps) + 2 * U                      # (+ alpha itself: 1/10 and 9/10 are rounded)
    for i in range(5):
        for j in range(5):
            exact = want[i][j]
            if exact == 0:
                assert got[i, j] == 0.0
            else:
                assert abs(Fraction(float(got[i, j])) - exact) <= Fraction(bound) * exact, (i, j)


# ----------------------------------------------------------------------------------------------------- resolvent ----

def _inverse_longdouble(a):
    """Gauss-Jordan with partial pivoting in np.longdouble (np.linalg.inv has no such path)."""
    n = a.shape[0]
    m = np.concatenate([a.astype(np.longdouble), np.eye(n, dtype=np.longdouble)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        m[[c, p]] = m[[p, c]]
        m[c] = m[c] / m[c, c]
        for r in range(n):
            if r != c:
                m[r] = m[r] - m[r, c] * m[c]
    return m[:, n:]


def test_kernel_tends_to_the_resolvent():
    """K_T against alpha inv(I - beta S) on a weighted 40-node graph at alpha = beta = 1/2, T = 41.
    Truncation: alpha inv(I - beta S) - K_T = (beta S)^T (alpha inv(I - beta S) - I); S is symmetric with spectrum in [-1, 1], and
    |alpha / (1 - beta x) - 1| <= 1 there, so every element differs by at most beta^T = 4.5e-13 (and beta^(T+1) = 2.3e-13), below
    1e-12.  Rounding: the f64 run against the same restatement in np.longdouble differs by at most 5.7e-17 in any element (measured
    once, on this graph; elements are below 1); allowed with a factor 4: 2.3e-16.  The inverse is taken in np.longdouble too."""
    n, steps, alpha = 40, 41, 0.5
    eu, ev, w = dr.random_sparse(n, 5, 3)
    k = dr.kernel(n, eu, ev, w, alpha, steps)
    k_long = dr.kernel(n, eu, ev, w, alpha, steps, np.longdouble)
    measured = float(np.abs(k - k_long).max())
    print('f64 run against the longdouble run: max |difference| = %.3g' % measured)
    assert measured <= 4 * 5.7e-17
    ptr, col, wt = dr.csr(n, eu, ev, w)
    _, s = dr.scaled(ptr, col, wt, np.longdouble)
    dense = np.zeros((n, n), dtype=np.longdouble)
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(ptr)), col), s)
    resolvent = np.longdouble(alpha) * _inverse_longdouble(np.eye(n, dtype=np.longdouble) - np.longdouble(1 - alpha) * dense)
    truncation = (1 - alpha) ** steps
    assert truncation < 1e-12 and (1 - alpha) ** (steps + 1) < 1e-12
    assert float(np.abs(k - resolvent).max()) <= truncation + 4 * 5.7e-17


# --------------------------------------------------------------------------------------------------- closed form ----

@pytest.mark.parametrize('n,alpha,steps', [(12, Fraction(1, 2), 10), (7, Fraction(1, 10), 5), (5, Fraction(9, 10), 32)])
def test_complete_graph_closed_form(n, alpha, steps):
    """S = (J - I) / (n - 1) has the eigenvalue 1 on the constant vector and -1 / (n - 1) elsewhere, so with
    g(x) = alpha (1 - (beta x)^T) / (1 - beta x) + (beta x)^T:  K = g(1) J / n + g(-1 / (n - 1)) (I - J / n)."""
    beta = 1 - alpha

    def g(x):
        m = beta * x
        return alpha * (1 - m ** steps) / (1 - m) + m ** steps
    g1, g2 = g(Fraction(1)), g(Fraction(-1, n - 1))
    diag, off = g1 / n + g2 * (1 - Fraction(1, n)), (g1 - g2) / n
    eu, ev = np.triu_indices(n, 1)
    k = dr.kernel(n, eu, ev, None, float(alpha), steps)
    bound = Fraction(rounding_bound(n - 1, steps) + 2 * U)
    for i in range(n):
        for j in range(n):
            exact = diag if i == j else off
            assert abs(Fraction(float(k[i, j])) - exact) <= bound * exact, (i, j)
    d = dr.distance(k)
    want = 1 - float(off / diag)
    assert np.allclose(d[~np.eye(n, dtype=bool)], want, rtol=0, atol=4 * float(bound))


# ---------------------------------------------------------------------------------------------------- properties ----

def check_distance_matrix(d):
    assert np.array_equal(d, d.T) and not d.diagonal().any()
    finite = np.isfinite(d)
    assert ((d[finite] >= 0) & (d[finite] <= 1)).all() and np.isposinf(d[~finite]).all()


@pytest.mark.parametrize('steps', [1, 3, 8])
def test_a_path_is_reached_exactly_up_to_T_hops(steps):
    n = 24
    eu, ev = dr.path_graph(n)
    d = dr.distance(dr.kernel(n, eu, ev, None, 0.5, steps))
    check_distance_matrix(d)
    hop = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    assert np.array_equal(np.isfinite(d), hop <= steps)


def test_components_and_isolated_nodes_are_unreached():
    n = 31
    eu, ev, w = dr.awkward_graph(n, 5)
    d = dr.distance(dr.kernel(n, eu, ev, w, 0.5, 32))
    check_distance_matrix(d)
    half = (n - 1) // 2
    comp = np.where(np.arange(n) < half, 0, 1)
    comp[n - 1] = 2
    same = comp[:, None] == comp[None, :]
    assert np.isposinf(d[~same]).all()
    assert np.isposinf(np.delete(d[n - 1], n - 1)).all() and d[n - 1, n - 1] == 0.0
    assert np.isfinite(d[:half, :half]).all() and np.isfinite(d[half:n - 1, half:n - 1]).all()
    a = dr.members(d, 0.3)
    assert a.diagonal().all() and np.array_equal(a == 1, (d <= 0.3) | np.eye(n, dtype=bool))
    assert np.array_equal(np.isfinite(dr.kept(d, 0.3)), a == 1)


@pytest.mark.parametrize('graph', ['ring', 'grid'])
@pytest.mark.parametrize('k', [4, 8])
def test_the_nearest_nodes_are_hop_nearest(graph, k):
    """At the default parameters the k nearest nodes under D have the k smallest hop distances.  k = 4 and 8: the first two hop
    shells of a node of the ring lattice (4 + 4) and the first shell and most of the second (4 + 8) of an interior grid node.  This
    is not a theorem at any k: on the bounded grid at k = 20 a well-connected interior node at 4 hops can come before a corner
    at 3 hops -- path multiplicity is what the distance is meant to reward."""
    n, (eu, ev) = (60, dr.ring_lattice(60, 2)) if graph == 'ring' else (81, dr.grid_graph(9, 9))
    d = dr.distance(dr.kernel(n, eu, ev, None, 0.5, 32))
    check_distance_matrix(d)
    hop = dr.hops(n, eu, ev)
    for i in range(n):
        order = np.argsort(d[i], kind='stable')
        nearest = order[order != i][:k]
        assert np.sort(hop[i, nearest]).tolist() == np.sort(np.delete(hop[i], i))[:k].tolist(), i


def test_more_paths_are_nearer_at_equal_hops():
    """x and y are both two hops from node 0 and have the same degree and neighbors of the same degrees; three of x's neighbors are
    also neighbors of 0, only one of y's is."""
    #  0 - 1, 2, 3, 4 ;  x = 5 - 1, 2, 3 ;  y = 6 - 4, 7, 8 ;  7, 8 padded to the degree of 1, 2, 3 by a leaf each
    eu = np.array([0, 0, 0, 0, 5, 5, 5, 6, 6, 6, 7, 8])
    ev = np.array([1, 2, 3, 4, 1, 2, 3, 4, 7, 8, 9, 10])
    n = 11
    hop = dr.hops(n, eu, ev)
    assert hop[0, 5] == hop[0, 6] == 2
    for alpha in (0.1, 0.5, 0.9):
        d = dr.distance(dr.kernel(n, eu, ev, None, alpha, 32))
        assert d[0, 5] < d[0, 6]


# ------------------------------------------------------------------------------------ settings, INI keys, pickling ----

def test_settings_defaults_and_validation():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    assert (sf.diffusion_restart, sf.diffusion_steps) == (0.5, 32) and sf.node_distance_metric == 'shortpath_weighted_layout'
    sf.node_distance_metric = 'diffusion'
    sf.validate_config()
    assert sf.node_distance_metric == 'diffusion'
    sf.node_distance_metric = 'manhattan'
    with pytest.raises(ValueError, match='manhattan is not a valid setting for node_distance_metric'):
        sf.validate_config()
    assert sf.node_distance_metric == 'shortpath_weighted_layout'
    for bad in (0, 1, 0.0, 1.0, -0.2, 1.5, float('nan'), '0.5', None, True):
        sf.diffusion_restart = bad
        with pytest.raises(ValueError, match='diffusion_restart'):
            sf.validate_config()
        assert sf.diffusion_restart == 0.5
    for bad in (0, -3, 2.0, 1.5, '32', None, True):
        sf.diffusion_steps = bad
        with pytest.raises(ValueError, match='diffusion_steps'):
            sf.validate_config()
        assert sf.diffusion_steps == 32
    sf.diffusion_restart, sf.diffusion_steps = np.float64(0.25), np.int64(7)
    sf.validate_config()


def test_ini_keys(tmp_path):
    import safepy_amd
    ini = tmp_path / 'safe.ini'
    ini.write_text('[Analysis parameters]\nnodeDistanceType = diffusion\nneighborhoodRadiusType = percentile\nneighborhoodRadius = 1\n'
                   'diffusionRestart = 0.3\ndiffusionSteps = 12\n')
    sf = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert (sf.node_distance_metric, sf.diffusion_restart, sf.diffusion_steps) == ('diffusion', 0.3, 12)
    ini.write_text('[Analysis parameters]\nnodeDistanceType = diffusion\n')
    sf = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)                  # the keys are optional
    assert (sf.diffusion_restart, sf.diffusion_steps) == (0.5, 32)
    ini.write_text('[Analysis parameters]\ndiffusionSteps = many\n')
    with pytest.raises(ValueError, match="diffusion_steps = 'many'"):
        safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    ini.write_text('[Analysis parameters]\ndiffusionRestart = 1.0\n')
    with pytest.raises(ValueError, match='diffusion_restart = 1.0'):
        safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)


def test_settings_pickle_and_old_pickles_load_with_the_defaults():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.node_distance_metric, sf.diffusion_restart, sf.diffusion_steps = 'diffusion', 0.2, 5
    back = pickle.loads(pickle.dumps(sf))
    assert (back.node_distance_metric, back.diffusion_restart, back.diffusion_steps) == ('diffusion', 0.2, 5)
    state = sf.__getstate__()
    del state['diffusion_restart'], state['diffusion_steps']                        # an object pickled before the settings existed
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert (old.diffusion_restart, old.diffusion_steps) == (0.5, 32)
    old.validate_config()


# ------------------------------------------------------------------------------------------ refusals without a device ----

def _ring_graph(n=12, directed=False):
    import networkx as nx
    g = nx.DiGraph() if directed else nx.Graph()
    for i in range(n):
        g.add_node(i, x=float(np.cos(i)), y=float(np.sin(i)))
    for i in range(n):
        g.add_edge(i, (i + 1) % n)
    return g


def test_diameter_is_refused_before_any_device_work():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = _ring_graph()
    sentinel = np.eye(12, dtype=np.int64)
    sf._neighborhoods_host = sentinel
    for kind in ('diameter', None):
        sf.neighborhood_radius_type = kind
        with pytest.raises(ValueError, match="'diameter' is not defined for node_distance_metric = 'diffusion'"):
            sf.define_neighborhoods(node_distance_metric='diffusion')
        assert sf._neighborhoods_host is sentinel and sf._nbr is None
        with pytest.raises(ValueError, match="'diameter' is not defined"):
            sf.compute_node_distances()
        assert sf._node_distances is None
    with pytest.raises(ValueError, match='diffusion_restart'):
        sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='percentile', neighborhood_radius=1,
                                diffusion_restart=1.0)
    with pytest.raises(ValueError, match='diffusion_steps'):
        sf.define_neighborhoods(diffusion_steps=0)
    assert (sf.diffusion_restart, sf.diffusion_steps) == (0.5, 32) and sf._neighborhoods_host is sentinel


def test_directed_graphs_are_refused():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = _ring_graph(directed=True)
    with pytest.raises(NotImplementedError, match='directed'):
        sf.define_neighborhoods(node_distance_metric='diffusion', neighborhood_radius_type='nearest', neighborhood_radius=3)


# ---------------------------------------------------------------------------------------------------------------- ABI ----

def test_symbols_in_header_binding_and_library():
    from safepy_amd import _lib, backend as be
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name, n_args in (('safe_nbr_diffusion', 11), ('safe_last_diffusion_stats', 4)):
        assert re.search(r'\bint %s\s*\(' % name, code), name
        assert hasattr(raw, name) and _lib.PROTOTYPES[name][0] is ctypes.c_int and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert '#define SAFE_HIP_ABI_VERSION 9' in header and _lib.ABI_VERSION == 9      # additive
    assert callable(be.Neighborhoods.diffusion) and callable(be.Context.last_diffusion_stats)
    # NULL arguments: refused without a device, *out untouched
    h = ctypes.c_void_p(0x1234)
    eu = np.zeros(1, dtype=np.int32)
    rc = _lib.lib.safe_nbr_diffusion(None, 4, 1, eu.ctypes.data, eu.ctypes.data, None, 0.5, 4, 1.0, None, ctypes.byref(h))
    assert rc == _lib.E_INVALID and h.value == 0x1234 and b'safe_nbr_diffusion' in _lib.lib.safe_last_error()
    assert _lib.lib.safe_last_diffusion_stats(None, None, None, None) == _lib.E_INVALID
