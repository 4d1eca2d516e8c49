"""safe_nbr_diffusion on the device against the NumPy restatement of its contract (tests/diffusion_ref.py): the kernel matrix K and
the kept distances bit for bit, the membership in its three forms, the selections and derived handles that read the kept matrix,
reproducibility, steady device memory and the refusals.

Sizes: 1, 2, 63 / 64 / 65 (the transform's tile and the word of the bit matrix), 3 / 4 / 5 (rows of a wave task), 15 / 16 / 17
(rows of a workgroup of the step kernel), 127 / 128 / 129 (columns of a wave task; 120 / 121 and 128 / 129 are also the two sides
of the pitch, n rounded up to 8), 255 / 256 / 257 and 511 / 513 (two and four column chunks), 600 at the full T = 32, and
2047 / 2048 / 2049 at T <= 4, which keeps the NumPy reference at seconds.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import diffusion_ref as dr                        # noqa: E402
import weights_ref as wr                          # noqa: E402

INF = np.inf


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


GRAPHS = {}


def graph(name, n):
    """(eu, ev, w) of a named graph, made once."""
    key = (name, n)
    if key not in GRAPHS:
        if name == 'random':
            GRAPHS[key] = dr.random_sparse(n, 6, 100 + n)
        elif name == 'unit':
            GRAPHS[key] = dr.random_sparse(n, 5, 200 + n, weighted=False)
        elif name == 'path':
            GRAPHS[key] = dr.path_graph(n) + (None,)
        elif name == 'star':
            GRAPHS[key] = dr.star_graph(n) + (None,)
        elif name == 'awkward':
            GRAPHS[key] = dr.awkward_graph(n, 300 + n)
    return GRAPHS[key]


REFS = {}


def reference(name, n, restart, steps):
    """(K, D) of the restatement, computed once per case and never changed."""
    key = (name, n, restart, steps)
    if key not in REFS:
        eu, ev, w = graph(name, n)
        k = dr.kernel(n, eu, ev, w, restart, steps)
        d = dr.distance(k)
        k.setflags(write=False)
        d.setflags(write=False)
        REFS[key] = (k, d)
    return REFS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_handle(nbr, d, cutoff):
    a = dr.members(d, cutoff)
    assert np.array_equal(bits(nbr.distances()), bits(dr.kept(d, cutoff))), 'kept distances'
    assert np.array_equal(nbr.to_dense(), a), 'membership'
    assert np.array_equal(nbr.row_counts(), a.sum(axis=1))
    row_ptr, col = nbr.csr()
    assert np.array_equal(row_ptr, np.concatenate([[0], np.cumsum(a.sum(axis=1))])) and np.array_equal(col, np.nonzero(a)[1])
    assert (nbr.n, nbr.nnz, nbr.max_row_count) == (a.shape[0], int(a.sum()), int(a.sum(axis=1).max()))


def run_case(be, ctx, name, n, restart, steps, cutoffs=(INF,)):
    eu, ev, w = graph(name, n)
    k, d = reference(name, n, restart, steps)
    for cutoff in cutoffs:
        nbr, got = be.Neighborhoods.diffusion(ctx, n, eu, ev, w, restart, steps, cutoff, want_kernel=True)
        try:
            assert np.array_equal(bits(got), bits(k)), 'K differs from the restatement (%s, n = %d)' % (name, n)
            check_handle(nbr, d, cutoff)
        finally:
            nbr.close()


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 120, 121, 127, 128, 129, 255, 256, 257, 511, 513, 600])
def test_random_sparse_full_steps(be, ctx, n):
    run_case(be, ctx, 'random', n, 0.5, 32)


@pytest.mark.parametrize('n,steps', [(1023, 3), (1025, 3), (2047, 4), (2048, 2), (2049, 4)])
def test_random_sparse_large(be, ctx, n, steps):
    run_case(be, ctx, 'random', n, 0.5, steps)


@pytest.mark.parametrize('n', [9, 65, 130])
def test_path_reach_boundary(be, ctx, n):
    run_case(be, ctx, 'path', n, 0.5, 8, cutoffs=(INF, 0.3))
    _, d = reference('path', n, 0.5, 8)
    hop = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    assert np.array_equal(np.isfinite(d), hop <= 8)


def test_star_with_a_hub_of_2048_entries(be, ctx):
    run_case(be, ctx, 'star', 2049, 0.5, 4, cutoffs=(INF, 0.3))


@pytest.mark.parametrize('n', [31, 130])
def test_components_isolated_node_loops_duplicates_zero_weight(be, ctx, n):
    run_case(be, ctx, 'awkward', n, 0.5, 32, cutoffs=(INF, 0.3, 0.0))


def test_unit_weights_are_the_null_pointer(be, ctx):
    n = 130
    eu, ev, _ = graph('unit', n)
    k, d = reference('unit', n, 0.5, 32)
    for w in (None, np.ones(len(eu))):
        nbr, got = be.Neighborhoods.diffusion(ctx, n, eu, ev, w, 0.5, 32, INF, want_kernel=True)
        try:
            assert np.array_equal(bits(got), bits(k))
            check_handle(nbr, d, INF)
        finally:
            nbr.close()


@pytest.mark.parametrize('restart', [0.1, 0.5, 0.9])
@pytest.mark.parametrize('steps', [1, 2, 32])
def test_parameters_and_cutoffs(be, ctx, restart, steps):
    """Members are exactly D <= cutoff (and the diagonal): cutoff 0 keeps the diagonal and pairs at distance 0."""
    run_case(be, ctx, 'awkward', 130, restart, steps, cutoffs=(0.0, 0.3, INF))
    run_case(be, ctx, 'random', 65, restart, steps, cutoffs=(0.0, 0.3, INF))


def test_selections_and_derived_handles_read_the_kept_matrix(be, ctx):
    n = 257
    eu, ev, w = graph('awkward', n)
    _, d = reference('awkward', n, 0.5, 32)
    src = be.Neighborhoods.diffusion(ctx, n, eu, ev, w, 0.5, 32, INF)
    try:
        upper = d[np.triu_indices(n, 1)]
        finite = np.sort(upper[np.isfinite(upper)])
        values, count = src.distance_select([])
        assert count == len(finite)
        ranks = [0, 1, len(finite) // 3, len(finite) // 2, len(finite) - 2, len(finite) - 1, 1]
        values, count = src.distance_select(ranks)
        assert count == len(finite) and np.array_equal(bits(values), bits(finite[ranks]))
        for k in (1, 7, 50, 10 ** 6):
            want = np.zeros(n)
            for i in range(n):
                cand = np.sort(np.delete(d[i], i))
                cand = cand[np.isfinite(cand)]
                want[i] = cand[min(k, len(cand)) - 1] if len(cand) else 0.0
            radii = src.row_distance_select(k)
            assert np.array_equal(bits(radii), bits(want)), k
            if k == 7:
                assert want[n - 1] == 0.0                             # the isolated node
                for keep in (True, False):
                    nbr = be.Neighborhoods.from_distances_rows(src, radii, keep_distances=keep)
                    try:
                        a = ((d <= radii[:, None]) & np.isfinite(d)).astype(np.int64)
                        assert np.array_equal(nbr.to_dense(), a) and a.diagonal().all()
                        if keep:
                            assert np.array_equal(bits(nbr.distances()), bits(np.where(a == 1, d, INF)))
                            nbr.set_weights_from_distances('triangular', radii)
                            indptr, indices = wr.csr_of(a)
                            want_w = wr.member_weights('triangular', wr.matrix_member_distances(d, indptr, indices), indptr, radii)
                            assert np.array_equal(bits(nbr.weights()), bits(want_w))
                    finally:
                        nbr.close()
        check_handle(src, d, INF)                                     # the source handle is left as it was
    finally:
        src.close()


def test_identical_calls_give_identical_bytes(be, ctx):
    n = 513
    eu, ev, w = graph('random', n)
    outs = []
    for _ in range(3):
        nbr, k = be.Neighborhoods.diffusion(ctx, n, eu, ev, w, 0.5, 32, 0.3, want_kernel=True)
        outs.append((k, nbr.distances(), nbr.to_dense()))
        nbr.close()
    for k, dist, a in outs[1:]:
        assert np.array_equal(bits(k), bits(outs[0][0])) and np.array_equal(bits(dist), bits(outs[0][1]))
        assert np.array_equal(a, outs[0][2])


def test_device_memory_is_steady_over_repeated_calls(be, ctx):
    n = 130
    eu, ev, w = graph('awkward', n)

    def once():
        be.Neighborhoods.diffusion(ctx, n, eu, ev, w, 0.5, 4, 0.3).close()
    once()
    before = be.device_live_alloc_count()
    for _ in range(3):
        once()
    assert be.device_live_alloc_count() == before


def test_stats_of_the_last_call(be, ctx):
    n = 129
    eu, ev, w = graph('random', n)
    be.Neighborhoods.diffusion(ctx, n, eu, ev, w, 0.5, 5, INF).close()
    steps_ms, steps, transform_ms = ctx.last_diffusion_stats()
    assert steps == 5 and steps_ms > 0 and transform_ms > 0
    assert ctx.last_kernel()[0] == 'k_diffusion_step' and ctx.last_kernel()[2] == 5


def test_every_refusal_writes_nothing(be, ctx):
    lib, E_INVALID, E_UNSUPPORTED = be._lib.lib, be._lib.E_INVALID, be._lib.E_UNSUPPORTED
    n = 9
    eu, ev = (np.ascontiguousarray(x, dtype=np.int32) for x in dr.path_graph(n))
    ones = np.ones(len(eu))
    live = be.device_live_alloc_count()

    def refused(code, n=n, eu=eu, ev=ev, w=None, restart=0.5, steps=4, cutoff=INF):
        kernel = np.full((9, 9), -7.0)
        h = C.c_void_p(0x5AFE)
        rc = lib.safe_nbr_diffusion(ctx.handle, n, len(eu), eu.ctypes.data, ev.ctypes.data, None if w is None else w.ctypes.data,
                                    restart, steps, cutoff, kernel.ctypes.data, C.byref(h))
        assert rc == code, (rc, lib.safe_last_error())
        assert h.value == 0x5AFE and (kernel == -7.0).all()
        assert b'safe_nbr_diffusion' in lib.safe_last_error()

    for restart in (0.0, 1.0, -0.1, 1.5, float('nan')):
        refused(E_INVALID, restart=restart)
    for steps in (0, -1):
        refused(E_INVALID, steps=steps)
    refused(E_INVALID, cutoff=float('nan'))
    for bad_id in (-1, n):
        bad = eu.copy()
        bad[3] = bad_id
        refused(E_INVALID, eu=bad)
        refused(E_INVALID, ev=bad)
    for bad_w in (-1.0, float('nan'), float('inf')):
        w = ones.copy()
        w[2] = bad_w
        refused(E_INVALID, w=w)
    refused(E_INVALID, n=0)
    refused(E_UNSUPPORTED, n=65537)
    assert be.device_live_alloc_count() == live
    zero = ones.copy()
    zero[2] = 0.0                                                     # zero is allowed: the path falls into two components
    nbr = be.Neighborhoods.diffusion(ctx, n, eu, ev, zero, 0.5, 32, INF)
    try:
        d = dr.distance(dr.kernel(n, eu, ev, zero, 0.5, 32))
        check_handle(nbr, d, INF)
        assert np.isposinf(d[:3, 3:]).all()
    finally:
        nbr.close()
