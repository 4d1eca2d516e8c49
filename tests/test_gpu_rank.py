"""Attributes.rank() (safe_attr_rank, safepy_amd/csrc/rank.hip) against scipy.stats.rankdata(method='average', axis=0,
nan_policy='omit') ON THE BITS: midranks are multiples of 0.5 far below 2^52, the kernel compares integer keys, so there is no
tolerance anywhere in this file.  Shapes, column kinds and the SciPy results come from tests/rank_ref.py (computed once per
session, read-only); T is the implementation's chunk (_lib.RANK_CHUNK), imported.  Needs an MI355X."""
import numpy as np
import pytest

import rank_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


def ranked(be, ctx, b):
    """rank() of from_host(b), downloaded; the source must come back unchanged."""
    src = be.AttributeMatrix.from_host(ctx, b)
    try:
        r = src.rank()
        try:
            assert r.dtype == np.float64 and (r.n, r.m) == (src.n, src.m)
            out = r.download(np.float64, order='F')
        finally:
            r.close()
        dt = np.float32 if b.dtype in (np.float32, np.uint8, np.bool_) else np.float64
        back = src.download(dt, order='C' if b.flags['C_CONTIGUOUS'] else 'F')
        assert np.array_equal(back, b.astype(dt), equal_nan=True), 'the source was modified'
    finally:
        src.close()
    return out


@pytest.mark.parametrize('n', rr.shapes_n())
def test_designed_columns_f64(be, ctx, n):
    """Every column kind of rank_ref.column_kinds at every n around the tile, the wave and the chunk, one whole row NaN."""
    got = ranked(be, ctx, rr.designed(n))
    want = rr.want_cached('designed', n)
    assert got.dtype == np.float64
    bad = [name for j, name in enumerate(rr.column_kinds(n)) if not np.array_equal(got[:, j], want[:, j], equal_nan=True)]
    assert not bad and rr.same(got, want), (n, bad)


def test_70001_rows(be, ctx):
    assert rr.same(ranked(be, ctx, rr.big()), rr.want_cached('big'))


@pytest.mark.parametrize('dtype,order', [('float32', 'F'), ('float32', 'C'), ('float64', 'C')])
def test_designed_columns_other_layouts(be, ctx, dtype, order):
    """f32 values (subnormals down to 1e-45, neighbours one f32 ulp apart) and C order, at 2 T + 1 rows."""
    n = 2 * rr.chunk() + 1
    b = np.array(rr.designed(n, dtype), order=order)
    assert rr.same(ranked(be, ctx, b), rr.want_cached('designed', n, dtype))


@pytest.mark.parametrize('m', [1, 63, 64, 65, 129])
@pytest.mark.parametrize('n', [1, 130])
def test_c_order_on_both_sides_of_the_transpose_tile(be, ctx, n, m):
    """k_rank_keys_tile turns 64 x 64 tiles; stages 2 and 3 take one column per workgroup, so the tile is the only grouping."""
    for dtype in ('float64', 'float32'):
        b = rr.tiled(n, m, dtype, 'C')
        assert rr.same(ranked(be, ctx, b), rr.want(b)), dtype


@pytest.mark.parametrize('order', ['C', 'F'])
def test_u8_source(be, ctx, order):
    n = rr.chunk() + 5
    b = np.array(np.random.default_rng(8).integers(0, 256, size=(n, 66)).astype(np.uint8), order=order)
    b[:, 1] = b[:, 1] < 128                                   # 0/1 bytes
    assert rr.same(ranked(be, ctx, b), rr.want(b))


def test_no_columns_means_no_handle(be, ctx):
    """m = 0: the library makes no handle for an empty matrix (safe_attr_create_*: 'empty matrix'), so there is none to rank."""
    from safepy_amd import SafeHipError
    with pytest.raises(SafeHipError, match='empty matrix'):
        be.AttributeMatrix.from_host(ctx, np.empty((5, 0)))
    assert rr.want(np.empty((5, 0))).shape == (5, 0)


def test_csc_source_with_missing_rows(be, ctx):
    import scipy.sparse as sp
    n = rr.chunk() + 70
    rng = np.random.default_rng(11)
    dense = np.where(rng.uniform(size=(n, 40)) < 0.05, np.round(rng.normal(size=(n, 40)), 1), 0.0)
    missing = rng.uniform(size=n) < 0.1
    dense[missing] = 0.0
    src = be.AttributeMatrix.from_sparse(ctx, sp.csc_matrix(dense), missing_rows=missing)
    try:
        r = src.rank()
        got = r.download(np.float64, order='F')
        r.close()
    finally:
        src.close()
    full = dense.copy()
    full[missing] = np.nan
    assert rr.same(got, rr.want(full))


def test_borrowed_device_source_on_a_busy_stream(be, ctx):
    """A from_device source that becomes valid only behind a delay on the caller's stream (the manner of
    tests/test_gpu_stream_order.py: poisoned input, a delay, the true values copied in behind it, the context switched to that
    stream): the kernels of safe_attr_rank must queue behind the producer.  The call synchronises (the header says so), so
    what is checked is its start and its result.  The stream is made with the HIP runtime the library runs on; the delay is
    a chain of 200 fills of 512 MB on it (about 0.15 ms each): orders of magnitude above a launch, and nothing that can hang."""
    import ctypes as C
    from safepy_amd import _lib
    hip = C.CDLL(_lib.HIP_RUNTIME_PRELOADED or 'libamdhip64.so')
    D2D, NOT_READY = 3, 600

    def ok(code):
        assert code == 0, 'HIP error %d' % code

    n = 2 * rr.chunk() + 1
    b = np.ascontiguousarray(rr.designed(n))                  # C order
    want = rr.want_cached('designed', n)
    ballast, staging, tensor = ctx.alloc(512 << 20), ctx.alloc(b.nbytes), ctx.alloc(b.nbytes)
    stream, done = C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)))
    ok(hip.hipEventCreate(C.byref(done)))
    src = be.AttributeMatrix.from_device(ctx, tensor.ptr, np.float64, n, b.shape[1], order='C', keepalive=tensor)
    try:
        staging.upload(b)
        tensor.upload(b)
        r = src.rank()
        quiet = r.download(np.float64, order='F')
        r.close()
        assert rr.same(quiet, want)
        ctx.sync()
        ctx.set_stream(stream.value)
        try:
            ok(hip.hipMemsetAsync(C.c_void_p(tensor.ptr), 0xFF, C.c_size_t(b.nbytes), stream))        # poison: NaN
            for _ in range(200):
                ok(hip.hipMemsetAsync(C.c_void_p(ballast.ptr), 1, C.c_size_t(ballast.nbytes), stream))
            ok(hip.hipEventRecord(done, stream))
            ok(hip.hipMemcpyAsync(C.c_void_p(tensor.ptr), C.c_void_p(staging.ptr), C.c_size_t(b.nbytes), D2D, stream))
            assert hip.hipEventQuery(done) == NOT_READY, 'the harness drained the busy stream before the call'
            r = src.rank()
            busy = r.download(np.float64, order='F')
            r.close()
        finally:
            ctx.set_stream(None)
            ok(hip.hipStreamSynchronize(stream))
        assert rr.same(busy, want)
        assert np.array_equal(tensor.download(b.shape), b, equal_nan=True), 'the source was modified'
    finally:
        src.close()
        ok(hip.hipEventDestroy(done))
        ok(hip.hipStreamDestroy(stream))
        for buf in (ballast, staging, tensor):
            buf.free()


def test_row_flags_are_the_sources(be, ctx):
    n = 300
    b = rr.tiled(n, 7, 'float64', 'F')
    b[5] = np.nan
    src = be.AttributeMatrix.from_host(ctx, b)
    try:
        r0 = src.rank()                                       # before the source has any flags: the new handle finds its own
        own = r0.row_flags()
        r0.close()
        natural = src.row_flags()
        assert np.array_equal(own, natural) and natural[5] == 0 and natural[n // 2] == 0      # (rank_ref.designed: row n // 2 is NaN)
        assert natural.sum() == n - 2
        r1 = src.rank()                                       # computed flags
        assert np.array_equal(r1.row_flags(), natural)
        r1.close()
        installed = natural.copy()                            # a column shard: rows the full matrix has values in, and one it has not
        installed[[5, 17]] = [1, 0]
        src.set_row_flags(installed)
        r2 = src.rank()
        try:
            assert np.array_equal(r2.row_flags(), installed)
            assert r2.stats()['n_rows_with_value'] == int(installed.sum())
            assert np.array_equal(r2.row_flags(), installed)  # (the statistics pass keeps installed flags)
        finally:
            r2.close()
    finally:
        src.close()


def test_ranked_handle_is_from_host_of_r(be, ctx):
    """stats, column sums and column moments of the ranked handle equal those of from_host(R), R in the handle's own (Fortran)
    order -- the contract says 'no later call can tell it from safe_attr_create_host of R', and the summation order of the
    moments follows the element order."""
    n = rr.chunk() + 9
    src = be.AttributeMatrix.from_host(ctx, rr.designed(n))
    r = src.rank()
    try:
        big_r = r.download(np.float64, order='F')
        twin = be.AttributeMatrix.from_host(ctx, big_r)
        try:
            assert r.stats() == twin.stats()
            assert np.array_equal(r.row_flags(), twin.row_flags())
            assert np.array_equal(r.column_sums(), twin.column_sums())
            for a, b in zip(r.column_moments(), twin.column_moments()):
                assert np.array_equal(a, b)
            assert np.array_equal(r.column_sums(), np.nansum(big_r, axis=0))      # (half-integers: exact in any order)
        finally:
            twin.close()
    finally:
        r.close()
        src.close()


def test_rank_of_ranks_is_the_same_matrix(be, ctx):
    n = 2 * rr.chunk() + 1
    src = be.AttributeMatrix.from_host(ctx, rr.designed(n))
    r1 = src.rank()
    r2 = r1.rank()
    try:
        assert rr.same(r2.download(np.float64, order='F'), rr.want_cached('designed', n))
    finally:
        r2.close()
        r1.close()
        src.close()


def test_device_memory_is_steady(be, ctx):
    """safe_live_alloc_count before and after: repeated calls and refusals leave no block behind (the first round fills the
    context's pool of small blocks and is not counted)."""
    import ctypes as C
    from safepy_amd import _lib
    b = rr.tiled(rr.chunk() + 3, 5, 'float32', 'C')
    src = be.AttributeMatrix.from_host(ctx, b)
    try:
        src.stats()

        def round_trip():
            r = src.rank()
            r.stats()
            r.close()
            h = C.c_void_p(0x1234)
            assert _lib.lib.safe_attr_rank(None, C.byref(h)) == _lib.E_INVALID and h.value in (None, 0x1234)
            assert _lib.lib.safe_attr_rank(src.handle, None) == _lib.E_INVALID
        round_trip()
        before = be.device_live_alloc_count()
        for _ in range(3):
            round_trip()
        assert be.device_live_alloc_count() == before
        r = src.rank()
        assert be.device_live_alloc_count() == before + 1     # R's block is the only allocation that survives
        r.close()
        assert be.device_live_alloc_count() == before
    finally:
        src.close()


def test_kernel_stats_name_the_three_kernels(be, ctx):
    src = be.AttributeMatrix.from_host(ctx, rr.designed(65))
    try:
        src.rank().close()
        name, ms, launches = ctx.last_kernel()
        assert name == 'k_rank_keys+k_rank_sort+k_rank_emit' and ms > 0
        parts = ctx.last_rank_stats()
        assert len(parts) == 3 and all(p > 0 for p in parts)
    finally:
        src.close()
