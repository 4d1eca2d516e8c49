"""The column-chunked exchange tail of the bit-sliced launch (enrich.hip: bits_tail_split, bits_tail_lists, the chunk launches of
bits_launch_spans) through the C API in one process: safe_set_exchange_chunks arms two chunks of 64 columns, SAFE_HIP_XCHG_TAIL
cuts the tail, and the same call with the tail unset is the reference -- the chunks' counters, the bounds, the callback and all
five output matrices, bit for bit.  Needs an MI355X; every case well under a second."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P = 300, 300
SWITCHES = ('SAFE_HIP_XCHG_TAIL', 'SAFE_HIP_XCHG_CHUNKS', 'SAFE_HIP_FORCE_PATH', 'SAFE_HIP_BITS_DBG', 'SAFE_HIP_BITS_SPAN', 'SAFE_HIP_STAGES')


@pytest.fixture(scope='module')
def lab():
    import safepy_amd
    from safepy_amd import backend as be
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    ctx = safepy_amd.Context.default(0)
    # neighborhoods of 0 .. ~200 members, one of them empty: below 1024 members and 8 (N + 1) < 65536, the blocked form
    rng = np.random.default_rng(20250311)
    size = rng.integers(1, 201, N)
    size[17] = 0
    a = np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        a[i, rng.choice(N, size[i], replace=False)] = 1
    nbr = be.Neighborhoods.from_dense(ctx, a)
    yield safepy_amd, be, ctx, nbr
    be.set_exchange_chunks(ctx, 0)
    nbr.close()


def attributes(m):
    rng = np.random.default_rng(1000 + m)
    b = (rng.uniform(size=(N, m)) < 0.2).astype(np.float64)
    b[rng.choice(N, 12, replace=False)] = np.nan
    return b


def run(be, ctx, nbr, b, nperm):
    """One safe_randomization: its five matrices and the enriched counts, the exported counters [m, n_pad], last_kernel()."""
    n, m = b.shape
    attr = be.Attributes.from_host(ctx, b)
    perms = be.Permutations(ctx, n, attr.row_flags(), nperm, 4711 + m)        # (a stream of its own per case: the first call draws it)
    outs = [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)]
    try:
        be.randomization(ctx, nbr, attr, perms, 'sum', 'both', 0.05, [o.ptr for o in outs])
        ctx.sync()
        stats = ctx.last_kernel()
        mats = [o.download((n, m)) for o in outs[:5]] + [outs[5].download((m,))]
    finally:
        for o in outs:
            o.free()
        perms.close()
        attr.close()
    n_pad, got_m, layout = be.packed_counts_info(ctx)
    assert (got_m, layout) == (m, 0)
    buf = ctx.alloc(4 * n_pad * m)
    try:
        be.export_packed_counts(ctx, buf.ptr, n_pad * m)
        ctx.sync()
        return mats, buf.download((m, n_pad), np.uint32), stats
    finally:
        buf.free()


def chunk(be, ctx, k, words):
    buf = ctx.alloc(4 * words)
    try:
        buf.upload(np.full(words, 0xA5A5A5A5, dtype=np.uint32))
        be.export_packed_chunk(ctx, k, buf.ptr, words)
        ctx.sync()
        return buf.download((words,), np.uint32)
    finally:
        buf.free()


def same_bits(got, want):
    return all(np.array_equal(g.view(np.uint64), w.view(np.uint64)) for g, w in zip(got, want))


@pytest.mark.parametrize('m, bounds', [(100, [0, 64, 100]), (40, [0, 40, 40])], ids=['ragged_second_chunk', 'empty_second_chunk'])
def test_tail_chunks_equal_the_call_without_a_tail(lab, monkeypatch, m, bounds):
    """Two chunks of 64 columns over m = 100 (64 + 36) and m = 40 (40 + none), tails of 0.4 of the permutations and of the last
    stage: chunk info, every chunk's counters, the outputs and the callback against the same call with the tail unset."""
    _, be, ctx, nbr = lab
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    b = attributes(m)
    want, whole, (name, _, launches) = run(be, ctx, nbr, b, P)
    assert name == 'k_permtest_bits_blk' and launches >= 3              # the blocked form, a drawn stream long enough for a tail
    assert be.packed_chunk_info(ctx)[0] == 0
    n_pad = whole.shape[1]
    calls = []
    tails = {}
    try:
        be.set_exchange_chunks(ctx, 2, 64, on_enqueued=lambda: calls.append(1))
        for frac in ('0.4', '1e-9'):
            monkeypatch.setenv('SAFE_HIP_XCHG_TAIL', frac)
            del calls[:]
            got, got_whole, (name, _, launches) = run(be, ctx, nbr, b, P)
            be.take_exchange_error(ctx)
            assert name == 'k_permtest_bits_blk' and launches >= 3 and len(calls) == 1
            made, got_bounds, tail_perms = be.packed_chunk_info(ctx)
            assert (made, got_bounds) == (2, bounds) and 1 <= tail_perms < P
            tails[frac] = tail_perms
            for k, (c0, c1) in enumerate(zip(bounds, bounds[1:])):
                words = 64 * n_pad + 32
                part = chunk(be, ctx, k, words)
                assert np.array_equal(part[:(c1 - c0) * n_pad], whole[c0:c1].ravel()) and not part[(c1 - c0) * n_pad:].any()
            assert np.array_equal(got_whole, whole) and same_bits(got, want)
        assert tails['1e-9'] <= tails['0.4']
    finally:
        monkeypatch.delenv('SAFE_HIP_XCHG_TAIL', raising=False)
        be.set_exchange_chunks(ctx, 0)


def test_too_few_launches_make_no_tail(lab, monkeypatch):
    """P = 60: fewer than three launches, so an armed tail is not cut -- no chunks, the results of the call without one."""
    _, be, ctx, nbr = lab
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    b = attributes(100)
    want, whole, (name, _, launches) = run(be, ctx, nbr, b, 60)
    assert name == 'k_permtest_bits_blk' and launches < 3
    calls = []
    try:
        be.set_exchange_chunks(ctx, 2, 64, on_enqueued=lambda: calls.append(1))
        monkeypatch.setenv('SAFE_HIP_XCHG_TAIL', '0.4')
        got, got_whole, _ = run(be, ctx, nbr, b, 60)
        assert be.packed_chunk_info(ctx)[0] == 0 and not calls
        assert np.array_equal(got_whole, whole) and same_bits(got, want)
    finally:
        monkeypatch.delenv('SAFE_HIP_XCHG_TAIL', raising=False)
        be.set_exchange_chunks(ctx, 0)
