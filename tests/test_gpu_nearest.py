"""neighborhood_radius_type = 'nearest' on the device: the per-row selection kernel (k_row_select, both key sources) and the
two per-row membership builders of nbr.hip against the NumPy restatement in tests/nearest_ref.py.  Every comparison is on
bits.  Needs an MI355X.

Edges of the selection kernel: one workgroup of 256 threads (four waves of 64) per row, a 2048-bin histogram per digit."""
import numpy as np
import pytest

import nearest_ref as nr
import radius_ref as rr
import shortpath_ref as sp

pytestmark = pytest.mark.gpu

GRAPH_SIZES = tuple(sorted(set(nr.SIZES) | {17}))                      # the sizes of the selection test, for the matrix source too


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


_EUCLID = {}


def euclid_case(kind, n):
    """(xy, D, sorted candidates) of one input, computed once and never changed."""
    if (kind, n) not in _EUCLID:
        xy = rr.xy_input(kind, n)
        d = nr.euclid(xy)
        for a in (xy, d):
            a.flags.writeable = False
        _EUCLID[(kind, n)] = (xy, d, nr.sorted_candidates(d, False))
    return _EUCLID[(kind, n)]


_GRAPHS = {}


def graph_case(n):
    """(graph, SciPy's unbounded Dijkstra matrix) of component_graph(n)."""
    if n not in _GRAPHS:
        g = nr.component_graph(n)
        d = sp.scipy_reference(g, np.inf)[1]
        d.flags.writeable = False
        _GRAPHS[n] = (g, d)
    return _GRAPHS[n]


def unbounded(amd, ctx, g):
    return amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, g.ew, np.inf, keep_distances=True)


def assert_forms(nbr, want):
    """to_dense, row_counts, csr, nnz and the widest row of a handle against the membership matrix `want`."""
    f = sp.forms(want)
    assert np.array_equal(nbr.to_dense(), want)
    assert np.array_equal(nbr.row_counts(), f['row_counts'])
    row_ptr, col = nbr.csr()
    assert np.array_equal(row_ptr, f['row_ptr']) and np.array_equal(col, f['col'])
    assert (nbr.nnz, nbr.max_row_count) == (f['nnz'], f['max_row_count'])


# ------------------------------------------------------------------ 1. selection from coordinates ----

@pytest.mark.parametrize('n', nr.SIZES)
@pytest.mark.parametrize('kind', rr.KINDS)
def test_select_rows_from_coordinates(ctx, kind, n):
    xy, _, sc = euclid_case(kind, n)
    for k in nr.ks_for(n):
        got = ctx.row_distance_select(xy, k)
        want = nr.radii_from_sorted(sc, k)
        bad = np.nonzero(nr.bits(got) != nr.bits(want))[0]
        assert bad.size == 0, (kind, n, k, bad[:5], got[bad[:5]], want[bad[:5]])


def test_select_rows_on_the_integer_lattice_every_k(ctx):
    xy = rr.xy_input('lattice', 64)
    sc = nr.sorted_candidates(nr.euclid(xy), False)
    assert np.unique(sc[0][:, :63]).size < 40                           # 63 candidates a row, a few dozen values: ties at most k
    for k in range(1, 64):
        assert np.array_equal(nr.bits(ctx.row_distance_select(xy, k)), nr.bits(nr.radii_from_sorted(sc, k))), k


def test_select_rows_square_root_tie_and_coincident_nodes(ctx):
    assert ctx.row_distance_select(nr.TIE_XY, 1)[0] == 1.0
    xy = np.array([(0.0, 0.0), (0.0, 0.0), (3.0, 4.0)])
    assert np.array_equal(ctx.row_distance_select(xy, 1), [0.0, 0.0, 5.0])         # left out by index, not by value
    assert np.array_equal(ctx.row_distance_select(xy[:1], 3), [0.0])                # a single node has no candidate


# ------------------------------------------------------------------ 2. selection from a kept matrix ----

@pytest.mark.parametrize('n', GRAPH_SIZES)
def test_select_rows_from_a_kept_matrix(amd, ctx, n):
    g, d = graph_case(n)
    sc = nr.sorted_candidates(d, True)
    nbr = unbounded(amd, ctx, g)
    try:
        assert np.array_equal(nr.bits(nbr.distances()), nr.bits(d))
        for k in nr.ks_for(n):
            assert np.array_equal(nr.bits(nbr.row_distance_select(k)), nr.bits(nr.radii_from_sorted(sc, k))), (n, k)
        far = nbr.row_distance_select(10 * n)                          # k larger than a component: its largest distance
        assert np.array_equal(nr.bits(far), nr.bits(np.where(np.isfinite(d), d, 0.0).max(axis=1)))
        if n >= 3:
            assert np.isinf(d[n - 1, :n - 1]).all() and far[n - 1] == 0.0 and nbr.row_distance_select(1)[n - 1] == 0.0
    finally:
        nbr.close()


@pytest.mark.parametrize('name', ['zero_mix', 'zero_components', 'loops_and_isolated', 'subnormal', 'no_edges', 'single_node',
                                  'two_nodes_apart', 'parallel_edges'])
def test_select_rows_on_designed_graphs(amd, ctx, name):
    """Zero-length edges, components whose every distance is 0.0, self loops, isolated nodes, subnormal lengths."""
    g = sp.edge_cases()[name][0]
    d = sp.oracle_reference(g, np.inf)[1]
    nbr = unbounded(amd, ctx, g)
    try:
        for k in (1, 2, 3, g.n, g.n + 5):
            r = nbr.row_distance_select(k)
            assert np.array_equal(nr.bits(r), nr.bits(nr.radii(d, k, True))), (name, k)
            out = amd.Neighborhoods.from_distances_rows(nbr, r, keep_distances=True)
            try:
                want = nr.membership(d, r, True)
                assert_forms(out, want)
                assert np.array_equal(nr.bits(out.distances()), nr.bits(nr.masked(d, want)))
            finally:
                out.close()
    finally:
        nbr.close()


# ------------------------------------------------------------------ 3. per-row membership ----

@pytest.mark.parametrize('n', nr.SIZES)
def test_euclidean_rows_forms(amd, ctx, n):
    for kind in ('uniform', 'far_node'):
        xy, d, sc = euclid_case(kind, n)
        for k in sorted({1, min(10, n), n - 1 if n > 1 else 1}):
            r = nr.radii_from_sorted(sc, k)
            nbr = amd.Neighborhoods.euclidean_rows(ctx, xy, r)
            try:
                assert_forms(nbr, nr.membership(d, r, False))
            finally:
                nbr.close()


@pytest.mark.parametrize('n', GRAPH_SIZES)
def test_from_distances_rows_forms_masked_matrix_and_untouched_source(amd, ctx, n):
    """The sizes of the selection test: 63 and 255 end in a partial word, 256 gives each of the builder's four waves exactly
    one word, 257 and beyond send a wave round its loop again."""
    g, d = graph_case(n)
    src = unbounded(amd, ctx, g)
    try:
        src_dense, src_counts = src.to_dense(), src.row_counts()
        for k in sorted({1, min(10, n), n}):
            r = nr.radii(d, k, True)
            want = nr.membership(d, r, True)
            kept = amd.Neighborhoods.from_distances_rows(src, r, keep_distances=True)
            bare = amd.Neighborhoods.from_distances_rows(src, r)
            try:
                assert_forms(kept, want)
                assert_forms(bare, want)
                assert np.array_equal(nr.bits(kept.distances()), nr.bits(nr.masked(d, want)))
                with pytest.raises(amd.SafeHipError):
                    bare.distances()
                # the new handle is a source like any other: its kept matrix answers the same selection inside the radii
                assert np.array_equal(nr.bits(kept.row_distance_select(k)), nr.bits(r))
            finally:
                kept.close()
                bare.close()
        assert np.array_equal(nr.bits(src.distances()), nr.bits(d))     # src_nbr is left as it was
        assert np.array_equal(src.to_dense(), src_dense) and np.array_equal(src.row_counts(), src_counts)
        assert np.array_equal(src.to_dense(), np.isfinite(d).astype(np.int64))
    finally:
        src.close()


def test_square_root_tie_membership(amd, ctx):
    d = nr.euclid(nr.TIE_XY)
    r = ctx.row_distance_select(nr.TIE_XY, 1)
    nbr = amd.Neighborhoods.euclidean_rows(ctx, nr.TIE_XY, r)
    try:
        got = nbr.to_dense()
        assert np.array_equal(got[0], [1, 1, 1, 0, 0])                  # squares 1 and 1 + 2^-52: one distance, both are members
        assert np.array_equal(got, nr.membership(d, nr.radii(d, 1, False), False))
    finally:
        nbr.close()
    below = np.full(5, np.nextafter(1.0, 0.0))                          # just under the tied distance: neither
    nbr = amd.Neighborhoods.euclidean_rows(ctx, nr.TIE_XY, below)
    try:
        assert np.array_equal(nbr.to_dense(), nr.membership(d, below, False)) and nbr.to_dense()[0].sum() == 1
    finally:
        nbr.close()


@pytest.mark.parametrize('n', [5, 65, 257])
def test_zero_infinite_and_subnormal_radii(amd, ctx, n):
    xy = rr.xy_input('uniform', n).copy()
    xy[3] = xy[1]                                                       # a coincident pair
    d = nr.euclid(xy)
    g, dg = graph_case(n)
    src = unbounded(amd, ctx, g)
    try:
        for r in (np.zeros(n), np.full(n, np.inf), np.full(n, 5e-324), np.full(n, 1e-310),
                  np.where(np.arange(n) % 2 == 0, 0.0, np.inf)):
            nbr = amd.Neighborhoods.euclidean_rows(ctx, xy, r)
            try:
                assert_forms(nbr, nr.membership(d, r, False))
            finally:
                nbr.close()
            nbr = amd.Neighborhoods.from_distances_rows(src, r, keep_distances=True)
            try:
                want = nr.membership(dg, r, True)
                assert_forms(nbr, want)
                assert np.array_equal(nr.bits(nbr.distances()), nr.bits(nr.masked(dg, want)))
            finally:
                nbr.close()
        zero = nr.membership(d, np.zeros(n), False)
        assert zero[1, 3] == zero[3, 1] == 1 and zero.sum() == n + 2    # radius 0: the diagonal and coincident nodes only
        assert nr.membership(d, np.full(n, np.inf), False).all()
        assert np.array_equal(nr.membership(dg, np.full(n, np.inf), True), np.isfinite(dg))      # everything reached, no more
    finally:
        src.close()


def test_overflowing_squares_with_an_infinite_radius(amd, ctx):
    xy = np.array([(0.0, 0.0), (1e200, 0.0), (1.0, 1.0), (-1e200, 1e200)])
    d = nr.euclid(xy)
    assert np.isinf(d[0, 1])                                            # pdist's own square overflows
    for k in (1, 2, 3):
        r = ctx.row_distance_select(xy, k)
        assert np.array_equal(nr.bits(r), nr.bits(nr.radii(d, k, False)))
        nbr = amd.Neighborhoods.euclidean_rows(ctx, xy, r)
        try:
            assert np.array_equal(nbr.to_dense(), nr.membership(d, r, False))
        finally:
            nbr.close()
    big = np.full(4, 1.7e308)                                           # a finite radius whose square overflows
    nbr = amd.Neighborhoods.euclidean_rows(ctx, xy, big)
    try:
        assert np.array_equal(nbr.to_dense(), nr.membership(d, big, False))
    finally:
        nbr.close()


def test_a_far_node_is_nobodys_neighbour_but_has_its_own(amd, ctx):
    n, k = 65, 4
    xy, d, sc = euclid_case('far_node', n)
    r = ctx.row_distance_select(xy, k)
    nbr = amd.Neighborhoods.euclidean_rows(ctx, xy, r)
    try:
        a = nbr.to_dense()
    finally:
        nbr.close()
    assert np.array_equal(a, nr.membership(d, nr.radii_from_sorted(sc, k), False))
    assert a[:, n - 1].sum() == 1 and a[n - 1].sum() >= k + 1           # only itself contains it; it contains k others (and ties)
    assert not np.array_equal(a, a.T)
