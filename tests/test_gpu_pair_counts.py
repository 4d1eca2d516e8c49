"""safe_enriched_pair_counts / safe_enriched_pair_counts_dev (include/safe_hip.h) against the NumPy restatement
tests/pair_counts_ref.py: q[a] = sum of W[i, j] over the ordered pairs of the nodes with value > 0 in column a, e[a] = their
number.  Exact integer equality everywhere.

The within-reach matrices W of the references come from outside the library: scipy's pdist for Euclidean handles, networkx's
bounded Dijkstra for shortest-path ones, the input matrix itself for from_dense handles (asymmetric, all zeros, identity).

Shapes are the smallest that reach every path of k_profile_pack<true> and k_pair_count (safepy_amd/csrc/domains.hip):
  WORD = 64 rows per bit word, PACK_COLS = 64 columns per pack workgroup, WAVE_COLS = 4 columns per count workgroup,
  CHUNK_ROWS = 1024 rows per row chunk (PC_CHUNK_WORDS = 16), LANE_ROWS = 4096 nodes per word a lane keeps (the count kernel
  is instantiated for KW = 1 .. 8 words per lane, KW = ceil(n / LANE_ROWS)), BLOCK_ROWS = 8 LANE_ROWS = 32 768 nodes per word
  block (PC_MAX_KW = 8), above which a column's words are split over blockIdx.z.
n runs over both sides of WORD, 2 WORD, CHUNK_ROWS and 2 CHUNK_ROWS, over every multiple of LANE_ROWS up to BLOCK_ROWS (the
first n of every KW) and over BLOCK_ROWS itself (from 4096 nodes on the reference is pdist on each column's enriched nodes: a
dense W would hold up to 10^9 entries); n_cols over both sides of WAVE_COLS, PACK_COLS and 4 PACK_COLS.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.distance import pdist

import pair_counts_ref as pc

pytestmark = pytest.mark.gpu

WORD, PACK_COLS, WAVE_COLS, CHUNK_ROWS, LANE_ROWS, BLOCK_ROWS = 64, 64, 4, 1024, 4096, 32768
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 1000, CHUNK_ROWS - 1, CHUNK_ROWS, CHUNK_ROWS + 1, 2049]
COLUMN_COUNTS = [1, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, PACK_COLS - 1, PACK_COLS, PACK_COLS + 1, 257]


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def ctx(amd):
    return amd.Context.default(0)


@pytest.fixture(scope='module')
def be():
    from safepy_amd import backend
    return backend


def on_device(ctx, host):
    buf = ctx.alloc_f64(*host.shape)
    buf.upload(np.ascontiguousarray(host, dtype=np.float64))
    return buf


def both_forms(ctx, be, nbr, values, cols):
    """(q, e) of the device form, after checking that the host form on the slice gives the same."""
    cols = np.asarray(cols, dtype=np.int64)
    n, m = values.shape
    buf = on_device(ctx, values)
    try:
        q, e, ms = be.enriched_pair_counts_dev(ctx, nbr, buf.ptr, n, m, cols)
    finally:
        buf.free()
    assert q.dtype == np.int64 and e.dtype == np.int64 and q.shape == e.shape == cols.shape
    assert ms > 0 and ctx.last_kernel()[0] == 'k_profile_pack+k_pair_count'
    qh, eh = be.enriched_pair_counts(ctx, nbr, values[:, cols])
    assert np.array_equal(q, qh) and np.array_equal(e, eh)
    return q, e


def layout(n, seed):
    return np.random.default_rng(seed).uniform(size=(n, 2))


# ------------------------------------------------------------------------------------------------- sizes and patterns ----

@pytest.mark.parametrize('n', SIZES)
def test_every_pattern_against_a_euclidean_relation(ctx, be, n):
    xy = layout(n, seed=n)
    t = 0.5 if n < 200 else 0.08
    values, names = pc.pattern_columns(n, seed=n + 1)
    cols = np.arange(values.shape[1])
    nbr = be.Neighborhoods.euclidean(ctx, xy, t)
    try:
        q, e = both_forms(ctx, be, nbr, values, cols)
    finally:
        nbr.close()
    want_q, want_e = pc.pair_counts(values, cols, pc.within_euclidean(xy, t))
    assert np.array_equal(e, want_e), dict(zip(names, zip(e.tolist(), want_e.tolist())))
    assert np.array_equal(q, want_q), dict(zip(names, zip(q.tolist(), want_q.tolist())))
    by = dict(zip(names, zip(q.tolist(), e.tolist())))
    assert by['empty'] == (0, 0) and by['one_node'] == (1, 1) and by['last_row'] == (1, 1) and by['full'][1] == n
    # only 1, 2.5 and +inf of {0, -0.0, 1, -1, 2.5, NaN, +inf, -inf} are enriched
    assert by['odd_values_cycle'][1] == int(pc.ODD_ENRICHED[np.arange(n) % 8].sum())
    pairs, within = pc.pairs_within(q, e)                                 # symmetric, full diagonal: the halving is exact
    assert (within <= pairs).all()


@pytest.mark.parametrize('n', [LANE_ROWS] + [k * LANE_ROWS + 1 for k in range(1, 8)] + [BLOCK_ROWS, BLOCK_ROWS + 70])
def test_every_width_of_the_count_kernel(ctx, be, n):
    """The last n of KW = 1, the first n of KW = 2 .. 8, the last n of one word block, and n above the 32 768 nodes one wave's
    registers cover: there the second word block holds 70 nodes."""
    rng = np.random.default_rng(n)
    xy = rng.uniform(size=(n, 2))
    t = 0.012 * np.sqrt(BLOCK_ROWS / n)                                  # ~15 nodes within reach at every n
    near = lambda i, rad: np.hypot(xy[:, 0] - xy[i, 0], xy[:, 1] - xy[i, 1]) < rad
    columns = [rng.uniform(size=n) < 0.01, near(n - 1, 4 * t), near(0, 3 * t) | near(n - 1, 3 * t), np.arange(n) % WORD == WORD - 1,
               np.arange(n) >= n - 70, np.arange(n) == n - 1, np.zeros(n, dtype=bool)]
    values = np.stack(columns, axis=1).astype(np.float64)
    values[~np.stack(columns, axis=1)] = pc.ODD_VALUES[~pc.ODD_ENRICHED][rng.integers(0, 5, size=int((~np.stack(columns, axis=1)).sum()))]
    cols = [0, 1, 2, 3, 4, 5, 6, 1]
    nbr = be.Neighborhoods.euclidean(ctx, xy, t)
    try:
        q, e = both_forms(ctx, be, nbr, values, cols)
    finally:
        nbr.close()
    for k, a in enumerate(cols):
        idx = np.flatnonzero(columns[a])
        assert e[k] == idx.size, a
        assert q[k] == idx.size + 2 * int((pdist(xy[idx]) < t).sum()) if idx.size > 1 else q[k] == idx.size, a
    assert q[1] > 3 * e[1] and q[4] >= e[4] == 70 and (q[5], e[5]) == (1, 1) and (q[6], e[6]) == (0, 0)


def test_column_counts_and_column_lists(ctx, be):
    n, m = 130, 260
    rng = np.random.default_rng(3)
    xy = layout(n, seed=4)
    t = 0.3
    patterns, _ = pc.pattern_columns(n, seed=5)
    values = (rng.uniform(size=(n, m)) < rng.uniform(0.0, 1.0, size=m)).astype(np.float64)
    values[:, :patterns.shape[1]] = patterns
    values[:, m - 1] = patterns[:, 1]                                      # the last column: full
    w = pc.within_euclidean(xy, t)
    lists = [np.arange(k) for k in COLUMN_COUNTS]
    lists += [np.arange(m - k, m) for k in (1, WAVE_COLS + 1, PACK_COLS + 1)]        # sub-ranges that end at the last column
    lists += [np.arange(100, 140), rng.permutation(m), rng.permutation(m)[:70], np.array([7, 7, 7, 7, 7]),
              np.array([m - 1, 0, m - 1, 3, 3, 259, 1]), rng.integers(0, m, size=257)]
    nbr = be.Neighborhoods.euclidean(ctx, xy, t)
    buf = on_device(ctx, values)
    try:
        for cols in lists:
            q, e, _ = be.enriched_pair_counts_dev(ctx, nbr, buf.ptr, n, m, cols)
            want_q, want_e = pc.pair_counts(values, cols, w)
            assert np.array_equal(q, want_q) and np.array_equal(e, want_e), cols
            qh, eh = be.enriched_pair_counts(ctx, nbr, values[:, cols])
            assert np.array_equal(qh, want_q) and np.array_equal(eh, want_e), cols
        q, e, ms = be.enriched_pair_counts_dev(ctx, nbr, buf.ptr, n, m, [])           # n_cols == 0: nothing to do
        assert q.shape == e.shape == (0,) and ms == 0
        q, e = be.enriched_pair_counts(ctx, nbr, np.zeros((n, 0)))
        assert q.shape == e.shape == (0,)
    finally:
        buf.free()
        nbr.close()


# ------------------------------------------------------------------------------------------------------- any handle ----

@pytest.mark.parametrize('n', [65, 129, CHUNK_ROWS + 1])
@pytest.mark.parametrize('kind', ['asymmetric', 'zeros', 'identity'])
def test_any_membership_matrix(ctx, be, n, kind):
    rng = np.random.default_rng(n)
    w = {'asymmetric': lambda: (rng.uniform(size=(n, n)) < 0.3).astype(np.int64), 'zeros': lambda: np.zeros((n, n), dtype=np.int64),
         'identity': lambda: np.eye(n, dtype=np.int64)}[kind]()
    if kind == 'asymmetric':
        assert not np.array_equal(w, w.T) and not np.diag(w).all()
    values, names = pc.pattern_columns(n, seed=n + 2)
    cols = np.arange(values.shape[1])
    nbr = be.Neighborhoods.from_dense(ctx, w)
    try:
        q, e = both_forms(ctx, be, nbr, values, cols)
    finally:
        nbr.close()
    want_q, want_e = pc.pair_counts(values, cols, w)
    assert np.array_equal(q, want_q) and np.array_equal(e, want_e)
    if kind == 'zeros':
        assert not q.any() and e.any()
    if kind == 'identity':
        assert np.array_equal(q, e)


@pytest.mark.parametrize('weight', ['length', 'hops'])
def test_shortest_path_relation_with_unreached_pairs(amd, ctx, be, weight):
    from safepy_amd.safe import _graph_arrays
    G, xy = pc.flow_graph(n=200, seed=21, lonely=15)
    n = 200
    _, eu, ev, length, _ = _graph_arrays(G)
    t = 0.35 if weight == 'length' else 3.0
    w = pc.within_shortpath(G, t, 'length' if weight == 'length' else 'weight')
    assert 0 < w.sum() < n * n and not w[0, n - 1]                        # the path on the last nodes is never reached
    values, _ = pc.pattern_columns(n, seed=22)
    cols = np.arange(values.shape[1])
    nbr = be.Neighborhoods.shortpath(ctx, n, eu, ev, length if weight == 'length' else None, t, keep_distances=False)
    try:
        q, e = both_forms(ctx, be, nbr, values, cols)
    finally:
        nbr.close()
    want_q, want_e = pc.pair_counts(values, cols, w)
    assert np.array_equal(q, want_q) and np.array_equal(e, want_e)
    pairs, within = pc.pairs_within(q, e)
    assert within[1] < pairs[1]                                           # 'full': the two components are out of reach


# ----------------------------------------------------------------------------------------------------- stream order ----

class Busy:
    """A caller's stream kept busy, as tests/test_gpu_domain_stage.py does for the siblings: the device input is poisoned, a
    chain of f32 4096 x 4096 matmuls of at least 30 ms is enqueued on the stream, the true input is copied in behind it on the
    same stream, and the entry point is called while the chain still runs (asserted)."""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx = torch, ctx
        self.s = torch.cuda.Stream()
        self.a = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device='cuda')
        self.c = torch.empty_like(self.a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            for _ in range(3):
                torch.mm(self.a, self.a, out=self.c)
            e0.record(self.s)
            for _ in range(4):
                torch.mm(self.a, self.a, out=self.c)
            e1.record(self.s)
        e1.synchronize()
        self.links = int(np.ceil(30.0 / max(e0.elapsed_time(e1) / 4.0, 0.02)))

    def run(self, t, staging, call):
        torch = self.torch
        torch.cuda.synchronize()
        self.ctx.set_stream(self.s.cuda_stream)
        try:
            with torch.cuda.stream(self.s):
                t.fill_(float('nan'))
                for _ in range(self.links):
                    torch.mm(self.a, self.a, out=self.c)
                done = torch.cuda.Event()
                done.record(self.s)
                t.copy_(staging)
            assert not done.query(), 'the harness drained the busy stream before the call: this would be a quiet run'
            out = call()
            with torch.cuda.stream(self.s):
                t.fill_(float('nan'))
            self.s.synchronize()
        finally:
            self.ctx.set_stream(None)
            torch.cuda.synchronize()
        return out


def test_counts_on_a_busy_stream(ctx, be):
    import torch
    assert torch.cuda.is_available()
    busy = Busy(ctx)
    n, m = 130, 70
    xy = layout(n, seed=31)
    values = (np.random.default_rng(32).uniform(size=(n, m)) < 0.4).astype(np.float64)
    values[:, 1] = 1
    staging = torch.from_numpy(values).cuda()
    t = torch.empty_like(staging)
    cols = [1, 3, 69, 3, 40]
    nbr = be.Neighborhoods.euclidean(ctx, xy, 0.3)
    try:
        q, e, _ = busy.run(t, staging, lambda: be.enriched_pair_counts_dev(ctx, nbr, t.data_ptr(), n, m, cols))
    finally:
        nbr.close()
    want_q, want_e = pc.pair_counts(values, cols, pc.within_euclidean(xy, 0.3))
    assert np.array_equal(q, want_q) and np.array_equal(e, want_e)
    assert e[0] == n                                                      # a NaN-poisoned column 1 would have no enriched node


# --------------------------------------------------------------------------------- refusals and device memory ----

def test_refusals_write_nothing_and_device_memory_is_steady(amd, ctx, be):
    from safepy_amd import _lib
    lib, h = _lib.lib, ctx.handle
    n, m = 65, 7
    xy = layout(n, seed=41)
    values = (np.random.default_rng(42).uniform(size=(n, m)) < 0.5).astype(np.float64)
    w = pc.within_euclidean(xy, 0.3)
    vp = C.c_void_p
    ptr = lambda a: vp(a.ctypes.data)
    nbr = be.Neighborhoods.euclidean(ctx, xy, 0.3)
    other = be.Neighborhoods.euclidean(ctx, layout(n + 1, seed=43), 0.3)
    buf = on_device(ctx, values)
    try:
        live = be.device_live_alloc_count()
        q, e = np.full(2, 12345, dtype=np.int64), np.full(2, 54321, dtype=np.int64)
        cols = np.array([0, 1], dtype=np.int64)

        def dev(hh=h, nb=nbr.handle, v=vp(buf.ptr), rows=n, width=m, c=cols, k=2, qq=q, ee=e):
            return lib.safe_enriched_pair_counts_dev(hh, nb, v, rows, width, ptr(c) if c is not None else None, k,
                                                     ptr(qq) if qq is not None else None, ptr(ee) if ee is not None else None, None)

        def host(hh=h, nb=nbr.handle, v=values[:, :2].copy(), k=2, qq=q, ee=e):
            return lib.safe_enriched_pair_counts(hh, nb, ptr(v) if v is not None else None, k, ptr(qq) if qq is not None else None,
                                                 ptr(ee) if ee is not None else None)
        for _ in range(3):
            # a column outside [0, m)
            for bad in ([0, m], [-1, 2], [3, 1 << 40]):
                assert dev(c=np.array(bad, dtype=np.int64)) == _lib.E_INVALID
                assert 'column' in lib.safe_last_error().decode()
            # NULL pointers: context, handle, matrix, column list, either output
            assert dev(hh=None) == _lib.E_INVALID and dev(nb=None) == _lib.E_INVALID and dev(v=None) == _lib.E_INVALID
            assert dev(c=None) == _lib.E_INVALID and dev(qq=None) == _lib.E_INVALID and dev(ee=None) == _lib.E_INVALID
            assert host(hh=None) == _lib.E_INVALID and host(nb=None) == _lib.E_INVALID and host(v=None) == _lib.E_INVALID
            assert host(qq=None) == _lib.E_INVALID and host(ee=None) == _lib.E_INVALID
            # n is not the handle's n; negative sizes
            assert dev(rows=n + 1) == _lib.E_INVALID and dev(nb=other.handle) == _lib.E_INVALID
            assert dev(rows=0) == _lib.E_INVALID and dev(width=-1) == _lib.E_INVALID and dev(k=-1) == _lib.E_INVALID
            assert host(k=-1) == _lib.E_INVALID
            assert (q == 12345).all() and (e == 54321).all()
            # n_cols == 0 succeeds and writes nothing, with or without pointers
            assert dev(k=0) == 0 and dev(k=0, c=None, qq=None, ee=None, v=None) == 0 and host(k=0) == 0 and host(k=0, v=None, qq=None, ee=None) == 0
            assert (q == 12345).all() and (e == 54321).all()
            with pytest.raises(amd.SafeHipError) as err:
                be.enriched_pair_counts_dev(ctx, nbr, buf.ptr, n, m, [0, m])
            assert err.value.code == _lib.E_INVALID
            with pytest.raises(ValueError):
                be.enriched_pair_counts(ctx, other, values)
            # and calls that succeed
            got_q, got_e, _ = be.enriched_pair_counts_dev(ctx, nbr, buf.ptr, n, m, [6, 0, 6])
            want_q, want_e = pc.pair_counts(values, [6, 0, 6], w)
            assert np.array_equal(got_q, want_q) and np.array_equal(got_e, want_e)
            got_q, got_e = be.enriched_pair_counts(ctx, nbr, values)
            assert np.array_equal(got_q, pc.pair_counts(values, np.arange(m), w)[0])
            assert be.device_live_alloc_count() == live
    finally:
        buf.free()
        nbr.close()
        other.close()
