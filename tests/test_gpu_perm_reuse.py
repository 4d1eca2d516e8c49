"""The resident table of a seeded permutation stream (rng.cpp, perms_create_impl).  The composed table is a pure function of
(seed, n, num_permutations, movable rows), and the last destroyed handle stays parked in its context with the complete table in
HBM: a seeded call with the same inputs takes that table instead of drawing, uploading, replaying and composing it again
(role 'resident' of Permutations.timing(), no draw time, the even launch spans of the device stream).  These tests pin

  * hit == miss: every output of the call and the table read back from the handle, bit for bit, against a call with
    SAFE_HIP_PERM_REUSE=0 and against NumPy's own stream;
  * every field of the key on its own (seed, one movable flag, P, N, random_seed=None), movable sets of equal size with other
    members, a handle abandoned before its stream was complete: all of them draw again and give what a reuse-off run gives;
  * another attribute block on the resident table (the run_batch pattern), a hit behind a busy caller stream, and no allocation
    on the hit path.

Comparisons are exact: counts are integers and the epilogue is deterministic, so no tolerance applies anywhere.

Shapes: N = 300 nodes with 7 all-NaN rows, M = 130 binary columns (three 64-attribute words, the last one partial).  P = 300:
the drawn stream runs in stages 16 | 48 | 128 | 76 | 32 (five launches), the resident table in even spans 200 | 100 (two);
P = 230: 16 | 48 | 128 | 38 against one launch of 230 (the 30-permutation tail joins its predecessor); P = 1.  The launch
counts are asserted: they are the stage plans of rng.cpp worked out by hand, not read off the library.

random_seed=None: with the device stream (the default) such a call generates its tables on the device and reports the role
'device'; with SAFE_HIP_DEVICE_STREAM=0 it runs the host stream from OS entropy (role 'own').  Neither may ever take or leave a
resident table; both are checked.

The busy-stream helpers (delay chain, poison) are those of tests/test_gpu_stream_order.py, restated here with an elementwise
link in the chain.
Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (radius rule only)

N, M, NAN_ROWS, SEED = 300, 130, 7, 5
OUTPUTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'num_neighborhoods_enriched')
# launches of the permutation kernel: (drawn stream, resident table) by P
LAUNCHES = {300: (5, 2), 230: (4, 1), 1: (1, 1)}


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    """A context of this module's own: fresh (nothing parked) when the first test starts, and no other module's handles in it."""
    return be.Context(0)


class Data:
    """Membership handles and attribute blocks of the module, built once."""

    def __init__(self, be, ctx):
        self.be, self.ctx = be, ctx
        self.nbr = {}
        for n in (N, N - 10):
            rng = np.random.default_rng(n)
            xy = rng.uniform(size=(n, 2))
            self.nbr[n] = be.Neighborhoods.euclidean(ctx, xy, orc.layout_radius(xy[:, 0], float(np.sqrt(10.0 / (np.pi * n)))))
        rng = np.random.default_rng(11)
        self.nan_rows = np.sort(rng.choice(N, NAN_ROWS, replace=False))
        self.b = self.block(rng, N, self.nan_rows)
        self.b_other = self.block(rng, N, self.nan_rows)                   # another attribute block, the same un-annotated rows
        free = np.setdiff1d(np.arange(N), self.nan_rows)
        self.b_more_nan = self.b.copy()                                    # one movable flag less
        self.b_more_nan[free[3]] = np.nan
        self.b_moved_nan = self.b.copy()                                   # as many NaN rows, one of them elsewhere
        self.b_moved_nan[self.nan_rows[0]] = self.b[free[5]]
        self.b_moved_nan[free[5]] = np.nan
        self.b_small = self.block(rng, N - 10, np.sort(rng.choice(N - 10, NAN_ROWS, replace=False)))
        self.refs = {}

    @staticmethod
    def block(rng, n, nan_rows):
        b = (rng.uniform(size=(n, M)) < 0.1).astype(np.float64)
        b[nan_rows] = np.nan
        return b

    def close(self):
        for nbr in self.nbr.values():
            nbr.close()


@pytest.fixture(scope='module')
def data(be, ctx):
    d = Data(be, ctx)
    yield d
    d.close()


def numpy_tables(n, flags, nperm, seed):
    """np.random.seed(seed); nperm x [perm = np.random.permutation(indx_vals); cur[indx_vals] = cur[perm]] -- the reference's loop."""
    np.random.seed(seed)
    movable = np.flatnonzero(flags)
    cur = np.arange(n)
    out = np.empty((nperm, n), dtype=np.int64)
    for q in range(nperm):
        perm = np.random.permutation(movable)
        cur[movable] = cur[perm]
        out[q] = cur
    return out


def forget(data):
    """Leaves a handle of another shape parked in the context: whatever table was resident is gone."""
    data.be.Permutations(data.ctx, 2, np.ones(2, dtype=np.uint8), 1, None, device_key=1).close()


def run(data, b, nperm=300, seed=SEED, device_key=None, held=None):
    """One compute_pvalues pass (row flags, permutation handle, safe_randomization) on the module's context: the six outputs,
    the table read back from the handle afterwards, the handle's timing and the kernel launches.  held: (attribute handle,
    output buffers) of the caller's own, kept across calls."""
    be, ctx = data.be, data.ctx
    n, m = b.shape
    attr, bufs = held or (be.Attributes.from_host(ctx, b), [ctx.alloc_f64(n, m) for _ in range(5)] + [ctx.alloc_f64(m)])
    flags = attr.row_flags()
    for buf in bufs:
        buf.zero()
    perms = be.Permutations(ctx, n, flags, nperm, seed, device_key=device_key)
    try:
        role_at_create = perms.timing()['role']
        be.randomization(ctx, data.nbr[n], attr, perms, 'sum', 'both', 0.05, [buf.ptr for buf in bufs])
        name, _, launches = ctx.last_kernel()
        timing = perms.timing()
        table = perms.read().astype(np.int64)
    finally:
        perms.close()
    outs = {k: buf.download((n, m) if i < 5 else (m,)) for i, (k, buf) in enumerate(zip(OUTPUTS, bufs))}
    if held is None:
        for buf in bufs:
            buf.free()
        attr.close()
    assert timing['role'] == role_at_create
    assert name == 'k_permtest_bits_blk', name
    return {'outs': outs, 'table': table, 'timing': timing, 'role': timing['role'], 'launches': launches, 'flags': flags}


def reference(data, monkeypatch, key, b, nperm=300, seed=SEED, device_key=None):
    """The same call with the resident table switched off, computed once per input set and shared."""
    if key not in data.refs:
        with monkeypatch.context() as mp:
            mp.setenv('SAFE_HIP_PERM_REUSE', '0')
            r = run(data, b, nperm, seed, device_key)
        assert r['role'] == ('own' if seed is not None else 'device')
        if seed is not None:
            np.testing.assert_array_equal(r['table'], numpy_tables(b.shape[0], r['flags'], nperm, seed))
        data.refs[key] = r
    return data.refs[key]


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint64)


def assert_same(got, want, what):
    for k in OUTPUTS:
        assert got['outs'][k].shape == want['outs'][k].shape, (what, k)
        assert np.array_equal(bits(got['outs'][k]), bits(want['outs'][k])), '%s: %s differs' % (what, k)
    np.testing.assert_array_equal(got['table'], want['table'], err_msg=what)


def differs(got, want):
    """The counts of two calls of one shape differ somewhere (another stream on the same data, or other data)."""
    return any(not np.array_equal(bits(got['outs'][k]), bits(want['outs'][k])) for k in ('pvalues_neg', 'pvalues_pos'))


# ------------------------------------------------------------------------------------------------------ hit == miss ----

@pytest.mark.parametrize('nperm', [300, 230, 1])
def test_hit_equals_miss(data, monkeypatch, nperm):
    """A: nothing resident (for P = 300 the module's fresh context), B: the same inputs, C: the same with SAFE_HIP_PERM_REUSE=0."""
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    if nperm != 300:
        forget(data)
    a = run(data, data.b, nperm)
    b = run(data, data.b, nperm)
    with monkeypatch.context() as mp:
        mp.setenv('SAFE_HIP_PERM_REUSE', '0')
        c = run(data, data.b, nperm)
    d = run(data, data.b, nperm)                                            # (C's own table is as good as A's)
    assert a['role'] == 'own' and a['timing']['draw_busy_ms'] > 0.0
    assert b['role'] == 'resident' and b['timing']['draw_busy_ms'] == 0.0 and b['timing']['drawn_all_ms'] == 0.0
    assert c['role'] == 'own' and c['timing']['draw_busy_ms'] > 0.0
    assert d['role'] == 'resident'
    want = numpy_tables(N, a['flags'], nperm, SEED)
    assert int((a['flags'] == 0).sum()) == NAN_ROWS
    for r, what in ((a, 'A'), (b, 'B'), (c, 'C'), (d, 'D')):
        np.testing.assert_array_equal(r['table'], want, err_msg=what)
        assert_same(r, a, what)
    drawn, resident = LAUNCHES[nperm]
    assert [a['launches'], b['launches'], c['launches'], d['launches']] == [drawn, resident, drawn, resident]
    if nperm == 300:
        data.refs.setdefault('base', c)


# ------------------------------------------------------------------------------------------- the key, field by field ----

def changed_inputs(data, what):
    """(attribute block, P, seed, device key, environment) of the call that differs from the base call in one field."""
    return {'seed': (data.b, 300, SEED + 1, None, {}),
            'flag': (data.b_more_nan, 300, SEED, None, {}),
            'P': (data.b, 299, SEED, None, {}),
            'N': (data.b_small, 300, SEED, None, {}),
            'unseeded': (data.b, 300, None, 77, {})}[what]


@pytest.mark.parametrize('what', ['seed', 'flag', 'P', 'N', 'unseeded'])
def test_each_key_field_invalidates_on_its_own(data, monkeypatch, what):
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    base = reference(data, monkeypatch, 'base', data.b)
    b, nperm, seed, key, _ = changed_inputs(data, what)
    want = reference(data, monkeypatch, what, b, nperm, seed, key)
    forget(data)
    first = run(data, data.b)
    assert first['role'] == 'own'
    assert run(data, data.b)['role'] == 'resident'                          # the table of the base call is resident and valid
    got = run(data, b, nperm, seed, key)
    assert got['role'] == ('device' if what == 'unseeded' else 'own'), got['role']
    assert_same(got, want, what)
    # ... and not what the stale table would have given
    if what == 'N':
        assert got['table'].shape != base['table'].shape
    else:
        if what != 'P':                                                     # (the stream of 299 permutations is the first 299 rows of the base stream)
            assert not np.array_equal(got['table'], base['table'])
        assert differs(got, base)
    # the key follows the last call: the base inputs are a miss now, and right again
    again = run(data, data.b)
    assert again['role'] == 'own'
    assert_same(again, base, what + ': base inputs afterwards')


def test_entropy_seeded_host_stream_is_never_resident(data, monkeypatch):
    """random_seed=None on the host stream (SAFE_HIP_DEVICE_STREAM=0): OS entropy stays fresh -- it neither takes the resident
    table of a seeded call nor leaves one, and two such calls differ."""
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    base = reference(data, monkeypatch, 'base', data.b)
    forget(data)
    assert run(data, data.b)['role'] == 'own'
    with monkeypatch.context() as mp:
        mp.setenv('SAFE_HIP_DEVICE_STREAM', '0')
        u1 = run(data, data.b, seed=None)
        u2 = run(data, data.b, seed=None)
    assert u1['role'] == 'own' and u2['role'] == 'own'
    assert u1['timing']['draw_busy_ms'] > 0.0 and u2['timing']['draw_busy_ms'] > 0.0
    assert not np.array_equal(u1['table'], base['table']) and not np.array_equal(u2['table'], u1['table'])
    after = run(data, data.b)
    assert after['role'] == 'own'
    assert_same(after, base, 'seeded call after entropy-seeded ones')


def test_same_flag_count_with_other_rows_is_a_miss(data, monkeypatch):
    """Movable sets of equal size but other members: a key on k, or on a weak hash of the flags alone, would reuse the table."""
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    base = reference(data, monkeypatch, 'base', data.b)
    want = reference(data, monkeypatch, 'moved', data.b_moved_nan)
    assert want['flags'].sum() == base['flags'].sum() and not np.array_equal(want['flags'], base['flags'])
    forget(data)
    assert run(data, data.b)['role'] == 'own'
    got = run(data, data.b_moved_nan)
    assert got['role'] == 'own'
    assert_same(got, want, 'moved NaN row')
    assert not np.array_equal(got['table'], base['table']) and differs(got, base)


@pytest.mark.parametrize('consumed', [0, 10])
def test_abandoned_handle_is_never_valid(data, monkeypatch, consumed):
    """A handle destroyed before all its stages were enqueued (untouched, or after a read of its first rows) holds part of a
    table: the next identical create draws again."""
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    base = reference(data, monkeypatch, 'base', data.b)
    forget(data)
    perms = data.be.Permutations(data.ctx, N, base['flags'], 300, SEED)
    if consumed:
        np.testing.assert_array_equal(perms.read(0, consumed).astype(np.int64), base['table'][:consumed])
    perms.close()
    got = run(data, data.b)
    assert got['role'] == 'own' and got['timing']['draw_busy_ms'] > 0.0
    assert_same(got, base, 'after an abandoned handle')
    assert run(data, data.b)['role'] == 'resident'


def test_another_matrix_on_the_resident_table(data, monkeypatch):
    """run_batch's pattern: one seed, one network, one attribute block after the other with the same un-annotated rows."""
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    base = reference(data, monkeypatch, 'base', data.b)
    want = reference(data, monkeypatch, 'other', data.b_other)
    forget(data)
    a = run(data, data.b)
    got = run(data, data.b_other)
    assert a['role'] == 'own' and got['role'] == 'resident' and got['timing']['draw_busy_ms'] == 0.0
    assert_same(a, base, 'first block')
    assert_same(got, want, 'second block on the resident table')
    assert differs(got, base)


def test_no_allocation_on_the_hit_path(data, monkeypatch):
    """Ten hit-path calls on one attribute handle and one set of output buffers: the library allocates nothing."""
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    be, ctx = data.be, data.ctx
    base = reference(data, monkeypatch, 'base', data.b)
    forget(data)
    attr = be.Attributes.from_host(ctx, data.b)
    bufs = [ctx.alloc_f64(N, M) for _ in range(5)] + [ctx.alloc_f64(M)]
    try:
        assert run(data, data.b, held=(attr, bufs))['role'] == 'own'
        assert run(data, data.b, held=(attr, bufs))['role'] == 'resident'      # (the first hit builds the task plan of the even spans)
        before = be.device_alloc_count()
        for i in range(10):
            r = run(data, data.b, held=(attr, bufs))
            assert r['role'] == 'resident'
            if i in (0, 9):
                assert_same(r, base, 'hit %d' % i)
        assert be.device_alloc_count() == before
    finally:
        for buf in bufs:
            buf.free()
        attr.close()


# ------------------------------------------------------------------------------------------------ busy caller stream ----

def poison(t):
    """NaN into f32 / f64 tensors, 0xFF bytes into integer ones."""
    if t.is_floating_point():
        t.fill_(float('nan'))
    else:
        import torch
        t.view(-1).view(torch.uint8).fill_(255)


class Lab:
    """The caller's side: a busy stream and the operand of the delay chain.  One link is an in-place f32 add over 256 MB (an
    elementwise kernel instead of the matmul of tests/test_gpu_stream_order.py: no BLAS library to load in this module); it is
    timed with events, and the chain is repeated until it lasts max(30 ms, 3 x T_call), capped at 300 ms."""

    def __init__(self, torch):
        self.torch = torch
        self.s = torch.cuda.Stream()
        self.a = torch.zeros(64 << 20, dtype=torch.float32, device='cuda')
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            for _ in range(3):
                self.a.add_(1.0)
            e0.record(self.s)
            for _ in range(4):
                self.a.add_(1.0)
            e1.record(self.s)
        e1.synchronize()
        self.link_ms = max(e0.elapsed_time(e1) / 4.0, 0.02)

    def delay(self, stream, t_call_ms):
        """Enqueues the chain on `stream`; returns the event recorded behind it."""
        want_ms = min(max(30.0, 3.0 * t_call_ms), 300.0)
        with self.torch.cuda.stream(stream):
            for _ in range(int(np.ceil(want_ms / self.link_ms))):
                self.a.add_(1.0)
            done = self.torch.cuda.Event()
            done.record(stream)
        return done


def test_hit_behind_a_busy_caller_stream(data, monkeypatch):
    """The hit-path call on a caller's stream that is still busy producing the attribute matrix: the handle is created (resident)
    and safe_randomization called while the delay runs; the matrix becomes valid only behind it, the outputs are consumed and
    poisoned on the same stream straight after the call.  A launch that waited only for the re-recorded stage events -- they
    complete at once -- and not for the caller's stream would read poison."""
    import time
    import torch
    monkeypatch.delenv('SAFE_HIP_PERM_REUSE', raising=False)
    be, ctx = data.be, data.ctx
    base = reference(data, monkeypatch, 'base', data.b)
    lab = Lab(torch)
    staging = torch.from_numpy(np.ascontiguousarray(data.b)).to('cuda')
    tensor = torch.empty_like(staging)
    outs = [torch.empty((N, M), dtype=torch.float64, device='cuda') for _ in range(5)] + [torch.empty((M,), dtype=torch.float64, device='cuda')]
    ptrs = [o.data_ptr() for o in outs]
    flags = base['flags']                                                      # (from the host values: reading them back would drain the stream)
    attr = be.Attributes.from_device(ctx, tensor.data_ptr(), np.float64, N, M, 'C', keepalive=tensor)
    closed = []

    def call():
        perms = be.Permutations(ctx, N, flags, 300, SEED)
        role = perms.timing()['role']
        be.randomization(ctx, data.nbr[N], attr, perms, 'sum', 'both', 0.05, ptrs)
        closed.append(perms)                                                   # (destroyed after the consumer: a destroy drains the streams)
        return role

    try:
        # quiet: complete inputs, the context on its own stream; the first call leaves the table, the second is the quiet hit
        forget(data)
        tensor.copy_(staging)
        torch.cuda.synchronize()
        assert call() == 'own'
        ctx.sync()
        closed.pop().close()
        t0 = time.perf_counter()
        assert call() == 'resident'
        ctx.sync()
        t_call_ms = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        quiet = [o.cpu().numpy() for o in outs]
        closed.pop().close()
        for k, q in zip(OUTPUTS, quiet):
            assert np.array_equal(bits(q), bits(base['outs'][k])), 'quiet hit: %s' % k
        # busy
        s = lab.s
        snaps = [torch.empty_like(o) for o in outs]
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        try:
            with torch.cuda.stream(s):
                for o in outs:
                    poison(o)
                poison(tensor)
            delay_done = lab.delay(s, t_call_ms)
            with torch.cuda.stream(s):
                tensor.copy_(staging)
            # the guard of the harness itself: nothing between the delay and the call may have drained the caller's stream
            assert not delay_done.query(), 'the harness drained the busy stream before the call: this would be a quiet run'
            role = call()
            with torch.cuda.stream(s):
                for snap, o in zip(snaps, outs):
                    snap.copy_(o)
                for o in outs:
                    poison(o)
                poison(tensor)
            s.synchronize()
        finally:
            ctx.set_stream(None)
            torch.cuda.synchronize()
        assert role == 'resident'
        for k, q, snap in zip(OUTPUTS, quiet, snaps):
            assert np.array_equal(bits(snap.cpu().numpy()), bits(q)), 'busy hit: %s differs from the quiet run' % k
    finally:
        for perms in closed:
            perms.close()
        attr.close()
