"""safe_pairs_create / safe_pairs_read / safe_pairs_destroy (include/safe_hip.h) and SAFE.enriched_pairs on the device:
the selected cells of a device-resident f64 [n, m] matrix as CSR / CSC arrays.

Expected values come from tests/pairs_ref.py (held to SciPy by tests/test_enriched_pairs_cpu.py) on host copies of the same
matrices; the comparison is exact -- indptr and indices with array_equal, data through a uint64 view.

Shapes: both sides of the 64 lanes of a step, of the constants below, odd m (rows that are not 16-byte aligned), more
than one workgroup.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pairs_ref
import pytest

pytestmark = pytest.mark.gpu

# the constants of safepy_amd/csrc/pairs.hip
WAVE = 64                   # columns of a step (by row), columns of a wave (by column)
WAVES_PER_GROUP = 4         # (row, chunk) or (block, column group) tasks per workgroup: PAIRS_THREADS / 64
ROW_STEP = 256              # columns whose loads are issued together: 64 * PAIRS_UNROLL
ROW_CHUNK = 2048            # PAIRS_ROW_CHUNK: columns of a row one wave walks
COL_ROWS = 64               # PAIRS_COL_ROWS: rows of a block (by column)
COLSCAN_THREADS = 256       # columns per workgroup of the column scan
SCAN_TILE = 4096            # counts one pass of the scan's workgroup covers

T05 = float(-np.log10(0.05))
T_PRESENT = 1.0             # occurs in every matrix (pairs_ref.special_values): cells equal to it are not beyond it
COMBOS = [(0, 0.0)] + [(mode, t) for mode in (1, 2, 3) for t in (0.0, T05, np.inf, T_PRESENT)]

SMALL_SHAPES = [(1, 1), (1, 2), (2, 1), (1, 63), (1, 64), (1, 65), (63, 1), (64, 1), (65, 1), (3, 127), (3, 128), (3, 129),
                (127, 3), (128, 3), (129, 3)]
LARGE_SHAPES = [(257, 255), (255, 257), (1000, 1001),
                (3, ROW_CHUNK - 1), (3, ROW_CHUNK), (3, ROW_CHUNK + 1), (5, 2 * ROW_CHUNK + 1),
                (2, SCAN_TILE - 1), (2, SCAN_TILE), (2, SCAN_TILE + 1),                   # by column: the scan runs over m
                (SCAN_TILE - 1, 2), (SCAN_TILE, 2), (SCAN_TILE + 1, 2)]                   # by row: over n * chunks
PATTERNS = ['nothing', 'everything', 'corners', 'lanes_0_63', 'full_row', 'full_column', 'checkerboard', 'random_0.001',
            'random_0.02', 'random_0.5']


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


def pattern_mask(name, n, m, rng):
    p = np.zeros((n, m), dtype=bool)
    if name == 'everything':
        p[:] = True
    elif name == 'corners':
        p[0, 0] = p[0, m - 1] = p[n - 1, 0] = p[n - 1, m - 1] = True
    elif name == 'lanes_0_63':
        p[:, 0::WAVE] = True
        p[:, WAVE - 1::WAVE] = True
    elif name == 'full_row':
        p[n // 2, :] = True
    elif name == 'full_column':
        p[:, m // 2] = True
    elif name == 'checkerboard':
        p[(np.add.outer(np.arange(n), np.arange(m)) % 2) == 0] = True
    elif name.startswith('random_'):
        p = rng.random((n, m)) < float(name.split('_')[1])
    return p


def selector_for(mask, mode, t, rng):
    """A matrix of random 64-bit patterns and special values whose selection under (mode, t) is `mask` (at t = inf nothing
    can be selected: the matrix is then all kinds of values that are not).  Cells that fall on the wrong side are drawn again
    from the special values of the right side."""
    raw = pairs_ref.special_values(rng, mask.shape)
    pool = pairs_ref.special_values(rng, (4096,), p_special=0.7)
    pool_sel = pairs_ref.selected(pool, mode, t)
    if not pool_sel.any():
        mask = np.zeros_like(mask)
    for want, side in ((True, pool[pool_sel]), (False, pool[~pool_sel])):
        wrong = (pairs_ref.selected(raw, mode, t) != want) & (mask == want)
        if wrong.any():
            raw[wrong] = side[rng.integers(0, side.shape[0], size=int(wrong.sum()))]
    assert np.array_equal(pairs_ref.selected(raw, mode, t), mask)
    return raw


def assert_same(got, want, what):
    indptr, indices, data = got[:3]
    assert indptr.dtype == np.int32 and indices.dtype == np.int32, what
    assert np.array_equal(indptr, want[0]), what
    assert np.array_equal(indices, want[1]), what
    if want[2] is None:
        assert data is None, what
    else:
        assert data.dtype == np.float64 and np.array_equal(pairs_ref.bits(data), pairs_ref.bits(want[2])), what


def run_shape(ctx, n, m, combos_of):
    rng = np.random.default_rng(n * 100003 + m)
    values = pairs_ref.special_values(rng, (n, m))
    d_sel, d_val = ctx.alloc_f64(n, m), ctx.alloc_f64(n, m)
    d_val.upload(values)
    try:
        for k, name in enumerate(PATTERNS):
            mask = pattern_mask(name, n, m, rng)
            for mode, t in combos_of(k):
                sel = selector_for(mask, mode, t, rng)
                d_sel.upload(sel)
                chosen = pairs_ref.selected(sel, mode, t)
                for axis in (0, 1):
                    what = (n, m, name, mode, t, axis)
                    indptr, indices, data = pairs_ref.compressed(chosen, values, axis)
                    major = np.repeat(np.arange((n, m)[axis]), np.diff(indptr))
                    own = sel[(major, indices) if axis == 0 else (indices, major)]
                    # values from another matrix, from the selector itself, and the pattern alone
                    assert_same(ctx.enriched_pairs(d_sel.ptr, d_val.ptr, n, m, mode, t, axis), (indptr, indices, data), what)
                    assert_same(ctx.enriched_pairs(d_sel.ptr, d_sel.ptr, n, m, mode, t, axis), (indptr, indices, own), what)
                    assert_same(ctx.enriched_pairs(d_sel.ptr, None, n, m, mode, t, axis), (indptr, indices, None), what)
    finally:
        d_sel.free()
        d_val.free()


@pytest.mark.parametrize('n,m', SMALL_SHAPES)
def test_designed_matrices_small(ctx, n, m):
    """Every pattern x every (mode, threshold) x both axes."""
    run_shape(ctx, n, m, lambda k: COMBOS)


@pytest.mark.parametrize('n,m', LARGE_SHAPES)
def test_designed_matrices_large(ctx, n, m):
    """Every pattern with three (mode, threshold) combinations each, rotating through all thirteen, both axes."""
    run_shape(ctx, n, m, lambda k: [COMBOS[(3 * k + j) % len(COMBOS)] for j in range(3)])


@pytest.mark.parametrize('n,m', [(1, 70001), (70001, 1)])
def test_long_rows_and_columns(ctx, n, m):
    """More than 65 535 entries in one row / one column: running counts wider than 16 bits."""
    sel = np.arange(1, n * m + 1, dtype=np.float64).reshape(n, m)
    d_sel = ctx.alloc_f64(n, m)
    d_sel.upload(sel)
    try:
        for axis in (0, 1):
            assert_same(ctx.enriched_pairs(d_sel.ptr, d_sel.ptr, n, m, 0, 0.0, axis), pairs_ref.compressed(sel > 0, sel, axis), (n, m, axis))
    finally:
        d_sel.free()


def test_cell_addresses_beyond_32_bits(ctx, be):
    """n = m = 46 342: 2.15e9 cells, just above 2^31.  Ones planted around linear index 2^31, in the last row and in the
    corners of a matrix of zeros made on the device; the expected arrays come from the planted positions."""
    import torch
    from safepy_amd import _lib
    n = m = 46342
    assert n * m > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip('the device reports %.1f GB free; the 17.2 GB selector needs 24 GB' % (free / 2 ** 30))
    cells = np.array([0, m - 1, 2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 2, 2 ** 31 + m,
                      (n - 1) * m, (n - 1) * m + 12345, n * m - 1], dtype=np.int64)
    rows, cols = cells // m, cells % m
    t = torch.zeros(n * m, dtype=torch.float64, device='cuda')
    try:
        t[torch.from_numpy(cells).cuda()] = 1.0
        torch.cuda.synchronize()
        for axis in (0, 1):
            major, minor = (rows, cols) if axis == 0 else (cols, rows)
            order = np.lexsort((minor, major))
            indptr = np.concatenate([[0], np.cumsum(np.bincount(major, minlength=n))]).astype(np.int32)
            got = ctx.enriched_pairs(t.data_ptr(), None, n, m, 0, 0.0, axis)
            assert_same(got, (indptr, minor[order].astype(np.int32), None), axis)
        # every cell selected (bytes 0x80: a negative number in every cell, below -0): nnz >= 2^31 is refused, with the number
        t.view(torch.uint8).fill_(0x80)
        torch.cuda.synchronize()
        live = be.device_live_alloc_count()
        with pytest.raises(_lib.SafeHipError) as err:
            ctx.enriched_pairs(t.data_ptr(), None, n, m, 3, 0.0, 0)
        assert err.value.code == _lib.E_UNSUPPORTED and str(n * m) in str(err.value)
        assert be.device_live_alloc_count() == live
    finally:
        del t
        torch.cuda.empty_cache()


def test_refusals_write_nothing(ctx, be):
    from safepy_amd import _lib
    lib = _lib.lib
    n, m = 70, 130
    rng = np.random.default_rng(3)
    sel = (rng.random((n, m)) < 0.2).astype(np.float64)
    d_sel = ctx.alloc_f64(n, m)
    d_sel.upload(sel)
    p_sel = C.c_void_p(d_sel.ptr)
    live = be.device_live_alloc_count()

    def create(ctx_h, sel_p, n_, m_, mode, t, axis, with_out=True, with_nnz=True):
        h, nnz, ms = C.c_void_p(), C.c_int64(-77), C.c_double()
        rc = lib.safe_pairs_create(ctx_h, sel_p, n_, m_, mode, t, axis, C.byref(h) if with_out else None,
                                   C.byref(nnz) if with_nnz else None, C.byref(ms))
        return rc, h, nnz.value, lib.safe_last_error().decode()

    for args, code, text in [
            ((None, p_sel, n, m, 0, 0.0, 0), _lib.E_INVALID, 'bad argument'),
            ((ctx.handle, p_sel, -1, m, 0, 0.0, 0), _lib.E_INVALID, 'bad argument'),
            ((ctx.handle, p_sel, n, -1, 0, 0.0, 0), _lib.E_INVALID, 'bad argument'),
            ((ctx.handle, None, n, m, 0, 0.0, 0), _lib.E_INVALID, 'selector_dev is NULL'),
            ((ctx.handle, p_sel, n, m, 4, 0.0, 0), _lib.E_INVALID, 'mode 4'),
            ((ctx.handle, p_sel, n, m, -1, 0.0, 0), _lib.E_INVALID, 'mode -1'),
            ((ctx.handle, p_sel, n, m, 0, 0.0, 2), _lib.E_INVALID, 'axis 2'),
            ((ctx.handle, p_sel, n, m, 0, 0.0, -1), _lib.E_INVALID, 'axis -1'),
            ((ctx.handle, p_sel, n, m, 1, float('nan'), 0), _lib.E_VALUE, 'threshold'),
            ((ctx.handle, p_sel, n, m, 2, -0.5, 1), _lib.E_VALUE, 'threshold'),
            ((ctx.handle, p_sel, n, m, 3, float('-inf'), 1), _lib.E_VALUE, 'threshold'),
            ((ctx.handle, p_sel, 2 ** 31, 1, 0, 0.0, 0), _lib.E_UNSUPPORTED, '[2147483648, 1]'),
            ((ctx.handle, p_sel, 1, 2 ** 31 + 5, 0, 0.0, 1), _lib.E_UNSUPPORTED, '[1, 2147483653]')]:
        rc, h, nnz, msg = create(*args)
        assert rc == code and text in msg, (args[2:], rc, msg)
        assert not h.value and nnz == -77
        assert be.device_live_alloc_count() == live
    assert create(ctx.handle, p_sel, n, m, 0, 0.0, 0, with_out=False)[0] == _lib.E_INVALID
    assert create(ctx.handle, p_sel, n, m, 0, 0.0, 0, with_nnz=False)[0] == _lib.E_INVALID
    assert be.device_live_alloc_count() == live

    # read: a good handle, bad arguments; pre-filled outputs stay as they are
    for axis in (0, 1):
        rc, h, nnz, _ = create(ctx.handle, p_sel, n, m, 0, 0.0, axis)
        assert rc == 0 and nnz == int(sel.sum()) > 0
        dim = (n, m)[axis]
        indptr, indices, data = np.full(dim + 1, -5, np.int32), np.full(nnz, -6, np.int32), np.full(nnz, -7.0)
        ms = C.c_double()
        ptr = be._ptr
        for args, text in [((None, p_sel, p_sel, ptr(indptr), ptr(indices), ptr(data)), 'NULL argument'),
                           ((h, p_sel, p_sel, None, ptr(indices), ptr(data)), 'NULL argument'),
                           ((h, None, p_sel, ptr(indptr), ptr(indices), ptr(data)), 'selector_dev is NULL'),
                           ((h, p_sel, p_sel, ptr(indptr), None, ptr(data)), 'indices_host is NULL'),
                           ((h, p_sel, p_sel, ptr(indptr), ptr(indices), None), 'values_dev without data_host')]:
            assert lib.safe_pairs_read(*args, C.byref(ms)) == _lib.E_INVALID
            assert text in lib.safe_last_error().decode()
            assert (indptr == -5).all() and (indices == -6).all() and (data == -7.0).all()
        # the pattern alone leaves data_host alone
        assert lib.safe_pairs_read(h, p_sel, None, ptr(indptr), ptr(indices), ptr(data), C.byref(ms)) == 0
        assert (data == -7.0).all()
        assert_same((indptr, indices, None), pairs_ref.compressed(sel > 0, None, axis), axis)
        assert lib.safe_pairs_read(h, p_sel, p_sel, ptr(indptr), ptr(indices), ptr(data), C.byref(ms)) == 0
        assert_same((indptr, indices, data), pairs_ref.compressed(sel > 0, sel, axis), axis)
        assert ms.value > 0 and ctx.last_kernel()[0] == ('k_pairs_rows<emit>', 'k_pairs_cols<emit>')[axis]
        assert lib.safe_pairs_destroy(h) == 0
        assert be.device_live_alloc_count() == live                              # a normal create / read / destroy
    assert lib.safe_pairs_destroy(None) == 0

    # an empty matrix: an empty result, no selector needed
    for n0, m0 in ((0, 5), (5, 0), (0, 0)):
        for axis in (0, 1):
            indptr, indices, data, ms = ctx.enriched_pairs(None, None, n0, m0, 0, 0.0, axis)
            assert indptr.dtype == np.int32 and np.array_equal(indptr, np.zeros((n0, m0)[axis] + 1)) and indices.shape == (0,)
            assert ms == (0.0, 0.0)
    assert be.device_live_alloc_count() == live
    d_sel.free()


@pytest.mark.parametrize('axis', [0, 1])
def test_changed_selector_is_refused_without_a_stray_store(ctx, be, axis):
    """The selector is overwritten between create and read -- denser, sparser, the same count elsewhere: SAFE_E_VALUE, the
    pre-filled outputs untouched; with the original matrix back the same handle reads correctly."""
    from safepy_amd import _lib
    n, m = 300, 2100                                           # several row blocks, two chunks per row
    rng = np.random.default_rng(11 + axis)
    sel = (rng.random((n, m)) < 0.02).astype(np.float64)
    values = pairs_ref.special_values(rng, (n, m))
    d_sel, d_val = ctx.alloc_f64(n, m), ctx.alloc_f64(n, m)
    d_sel.upload(sel)
    d_val.upload(values)
    live = be.device_live_alloc_count()
    pairs = be.Pairs(ctx, d_sel.ptr, n, m, 0, 0.0, axis)
    assert pairs.nnz == int(sel.sum())
    dim = (n, m)[axis]
    # every row / column keeps its count; the row chunks / row blocks do not where an entry crosses their border (at this
    # density a dozen entries do): only the clamp to the chunk's / block's own range keeps the entries of the others apart
    moved = np.roll(sel, 1, axis=1 - axis)
    assert not np.array_equal(pairs_ref.compressed(moved > 0, None, axis)[1], pairs_ref.compressed(sel > 0, None, axis)[1])
    edges = (np.arange(ROW_CHUNK, m, ROW_CHUNK), np.arange(COL_ROWS, n, COL_ROWS))[axis]
    assert np.take(moved, edges, axis=1 - axis).any(), 'no entry crosses a chunk / block border'
    for other in (np.ones((n, m)), (rng.random((n, m)) < 0.5).astype(np.float64), np.zeros((n, m)), sel * (rng.random((n, m)) < 0.5), moved):
        d_sel.upload(other)
        out = (np.full(dim + 1, -5, np.int32), np.full(pairs.nnz, -6, np.int32), np.full(pairs.nnz, -7.0))
        with pytest.raises(_lib.SafeHipError) as err:
            pairs.read(d_sel.ptr, d_val.ptr, out=out)
        assert err.value.code == _lib.E_VALUE and 'selection changed between create and read' in str(err.value)
        assert (out[0] == -5).all() and (out[1] == -6).all() and (out[2] == -7.0).all()
        assert out[1].shape == (pairs.nnz,)
    d_sel.upload(sel)
    assert_same(pairs.read(d_sel.ptr, d_val.ptr), pairs_ref.compressed(sel > 0, values, axis), axis)
    pairs.close()
    assert be.device_live_alloc_count() == live
    d_sel.free()
    d_val.free()


# ----------------------------------------------------------------------------------------------------- stream order ----

class Busy:
    """A caller's stream kept busy (the harness of tests/test_gpu_domain_stage.py): the device inputs are poisoned, a chain
    of f32 4096 x 4096 matmuls of at least 30 ms is enqueued on the stream, the true inputs are copied in behind it on the
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

    def run(self, inputs, call):
        """inputs: [(device tensor, staging tensor)]; returns call()'s result from the busy stream."""
        torch = self.torch
        torch.cuda.synchronize()
        self.ctx.set_stream(self.s.cuda_stream)
        try:
            with torch.cuda.stream(self.s):
                for t, _ in inputs:
                    t.fill_(float('nan'))
                for _ in range(self.links):
                    torch.mm(self.a, self.a, out=self.c)
                done = torch.cuda.Event()
                done.record(self.s)
                for t, staging in inputs:
                    t.copy_(staging)
            assert not done.query(), 'the harness drained the busy stream before the call: this would be a quiet run'
            out = call()
            with torch.cuda.stream(self.s):
                for t, _ in inputs:
                    t.fill_(float('nan'))
            self.s.synchronize()
        finally:
            self.ctx.set_stream(None)
            torch.cuda.synchronize()
        return out


@pytest.mark.parametrize('axis', [0, 1])
def test_pairs_on_a_busy_stream(ctx, be, axis):
    import torch
    assert torch.cuda.is_available()
    busy = Busy(ctx)
    n, m = 300, 2100
    rng = np.random.default_rng(5)
    sel = np.round(rng.normal(scale=1.5, size=(n, m)), 2)
    values = rng.random((n, m))
    staging = [torch.from_numpy(a).cuda() for a in (sel, values)]
    tensors = [torch.empty_like(s) for s in staging]
    d_sel, d_val = ctx.alloc_f64(n, m), ctx.alloc_f64(n, m)
    d_sel.upload(sel)
    d_val.upload(values)
    quiet = ctx.enriched_pairs(d_sel.ptr, d_val.ptr, n, m, 1, T05, axis)
    d_sel.free()
    d_val.free()
    assert quiet[1].shape[0] > 1000
    got = busy.run(list(zip(tensors, staging)),
                   lambda: be.enriched_pairs(ctx, tensors[0].data_ptr(), tensors[1].data_ptr(), n, m, 1, T05, axis))
    assert_same(got, quiet, axis)                              # (a NaN-poisoned selector would select nothing)
    assert_same(got, pairs_ref.compressed(np.abs(sel) > T05, values, axis), axis)


# ---------------------------------------------------------------------------------------------------------- drop-in ----

def resident(sf, names=('nes', 'nes_binary')):
    from safepy_amd.safe import _DeviceResult
    return [isinstance(sf.__dict__.get('_r_' + name), _DeviceResult) for name in names]


def small_instance(amd, how):
    from safepy_amd import workloads
    rng = np.random.default_rng(17)
    n, m = 300, 70
    xy = workloads.clustered_layout(rng, n)
    eu, ev = workloads.radius_edges(xy, 900, rng)
    length = np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1))
    # every attribute annotates the nodes nearest to a random one (so that neighborhoods are enriched) plus 2 % noise
    b = (rng.random((n, m)) < 0.02).astype(np.float64)
    for j in range(m):
        centre = xy[rng.integers(n)]
        b[np.argsort(((xy - centre) ** 2).sum(axis=1))[:rng.integers(5, 40)], j] = 1
    b[rng.choice(n, 12, replace=False)] = np.nan
    sf = amd.SAFE(verbose=False)
    sf.random_seed = 3
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=length)
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.2)
    sf.load_attributes(attribute_file=b)
    if how == 'randomization':
        sf.attribute_sign = 'both'
        sf.compute_pvalues(how='randomization', num_permutations=100)
    else:
        sf.compute_pvalues(how='hypergeometric')
    return sf


CALLS = [dict(values='nes'), dict(values='pvalues_pos'), dict(values=None), dict(values='nes_binary'),
         dict(values='nes', threshold=T05), dict(values='pvalues_pos', threshold=0.5, side='positive'),
         dict(values=None, threshold=0.0, side='negative'), dict(values='nes', threshold=0.0, side='negative')]


def arrays_of(a, fmt):
    return (a.row, a.col, a.data) if fmt == 'coo' else (a.indptr, a.indices, a.data)


@pytest.mark.parametrize('how', ['randomization', 'hypergeometric'])
def test_dropin_resident_equals_pairs_ref_and_host_path(amd, how):
    import scipy.sparse as sp
    sf = small_instance(amd, how)
    names = ('nes', 'nes_binary', 'pvalues_pos')
    assert resident(sf, names) == [True, True, True]
    got = {(k, fmt): sf.enriched_pairs(format=fmt, **kw) for k, kw in enumerate(CALLS) for fmt in ('csr', 'csc', 'coo')}
    table = sf.enriched_table()
    assert resident(sf, names) == [True, True, True], 'enriched_pairs downloaded or freed a result matrix'
    if how == 'randomization':
        assert resident(sf, ('ns', 'pvalues_neg')) == [True, True]
        neg = sf.enriched_pairs(values='pvalues_neg', threshold=0.0, side='negative')
        assert resident(sf, ('ns', 'pvalues_neg')) == [True, True]
    else:
        for name in ('ns', 'pvalues_neg'):
            with pytest.raises(ValueError, match=name):
                sf.enriched_pairs(values=name)
    sf.define_top_attributes()
    assert resident(sf) == [True, True], 'define_top_attributes left its resident path'

    # the matrices, read afterwards from the same instance
    mats = {name: getattr(sf, name) for name in names}
    assert resident(sf, names) == [False, False, False]
    assert mats['nes_binary'].sum() > 50
    if how == 'randomization':
        assert (mats['nes'] < 0).any()
        want = pairs_ref.pairs(mats['nes'], sf.pvalues_neg, pairs_ref.MODE_NEGATIVE, 0.0, 'csr')
        for g, w in zip(arrays_of(neg, 'csr'), want):
            assert np.array_equal(g, w)
    for (k, fmt), a in got.items():
        kw = CALLS[k]
        assert isinstance(a, {'csr': sp.csr_array, 'csc': sp.csc_array, 'coo': sp.coo_array}[fmt]) and a.shape == mats['nes'].shape
        threshold = kw.get('threshold')
        mode, t = (0, 0.0) if threshold is None else (pairs_ref.SIDE_MODES[kw.get('side', 'both')], threshold)
        selector = mats['nes_binary'] if threshold is None else mats['nes']
        want = pairs_ref.pairs(selector, None if kw['values'] is None else mats[kw['values']], mode, t, fmt)
        first, second, data = arrays_of(a, fmt)
        assert first.dtype == np.int32 and second.dtype == np.int32 and a.has_canonical_format
        assert np.array_equal(first, want[0]) and np.array_equal(second, want[1]), (kw, fmt)
        if kw['values'] is None:
            assert data.dtype == np.int8 and (data == 1).all() and data.shape == second.shape
        else:
            assert data.dtype == np.float64 and np.array_equal(pairs_ref.bits(data), pairs_ref.bits(want[2])), (kw, fmt)
        # ... and the same call on the host arrays
        host = sf.enriched_pairs(format=fmt, **kw)
        for g, h in zip(arrays_of(a, fmt), arrays_of(host, fmt)):
            assert g.dtype == h.dtype and np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                                                         h.view(np.uint64) if h.dtype == np.float64 else h), (kw, fmt)
    assert table.equals(sf.enriched_table())
    assert list(table.columns) == ['node', 'key', 'label', 'attribute', 'name', 'nes'] and len(table) == got[(0, 'coo')].nnz
