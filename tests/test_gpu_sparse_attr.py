"""A scipy.sparse node x attribute matrix as input: safe_attr_create_csc_host expands the stored entries on the device, and every
result must be BIT-IDENTICAL to the result for the dense equivalent.

The dense equivalent (include/safe_hip.h): 0 where nothing is stored, the stored value -- zeros and NaNs included -- where
something is, NaN across every row of `missing_rows`.  It is built here with NumPy from the CSC arrays (dense_equivalent), not
with .toarray(), so that the missing rows are part of it.  There is no tolerance anywhere in this file: handles are compared
with np.array_equal (equal_nan for the matrices), results bit for bit.

Shapes: the smallest that cross the boundaries the kernels have.  N = 70, M = 130 -- two 64-column words plus a tail, more rows
than a wave (k_csc_scatter: one wave per column; k_csc_validate: more than one workgroup of entries); N = 300, M = 70 -- above the
matrix cores' N >= 256 for the quantitative runs; and the degenerate ones: M = 1, nnz = 0, an empty first / middle / last column,
a completely full column, entries in row 0 and row N - 1 of column 0 and of column M - 1.

Allocation counts: backend.device_alloc_count() counts the hipMalloc / hipHostMalloc CALLS of the library ("a repeated call of
the same shape is expected to add none").  The create call takes every block from the context's pool and gives it back, so
after one warm-up cycle has filled the pool the counter must not move any more -- a block that was allocated and not returned
shows as one more call on the next cycle.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

RESULTS = ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')
NPERM, SEED, RADIUS = 20, 1, 0.2


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
def ctx(amd):
    return amd.Context.default(0)


# ------------------------------------------------------------------------------------------------------------- inputs ----

def csc_of_mask(mask):
    """(indptr int64 [m+1], indices int32 [nnz]) of a boolean [n, m] pattern: canonical CSC."""
    n, m = mask.shape
    cols = [np.flatnonzero(mask[:, j]).astype(np.int32) for j in range(m)]
    indptr = np.zeros(m + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(c) for c in cols])
    indices = np.concatenate(cols) if m else np.zeros(0, np.int32)
    return indptr, np.ascontiguousarray(indices, dtype=np.int32)


def pattern(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == 'n70_m130':
        n, m = 70, 130
        mask = rng.uniform(size=(n, m)) < 0.08
        mask[:, 5] = True                                   # a completely full column
        mask[:, 64] = False                                 # an empty middle column (first column of the third word's predecessor)
        for i, j in ((0, 0), (n - 1, 0), (0, m - 1), (n - 1, m - 1)):
            mask[i, j] = True
    elif name == 'n300_m70':
        n, m = 300, 70
        mask = rng.uniform(size=(n, m)) < 0.25
        mask[:, 33] = False
        for i, j in ((0, 0), (n - 1, 0), (0, m - 1), (n - 1, m - 1)):
            mask[i, j] = True
    elif name == 'm1':
        n, m = 70, 1
        mask = rng.uniform(size=(n, m)) < 0.2
        mask[0, 0] = mask[n - 1, 0] = True
    elif name == 'nnz0':
        n, m = 70, 3
        mask = np.zeros((n, m), dtype=bool)
    elif name == 'empty_first_last':
        n, m = 70, 130
        mask = rng.uniform(size=(n, m)) < 0.08
        mask[:, 0] = False
        mask[:, m - 1] = False
    else:
        raise KeyError(name)
    return n, m, mask


PATTERNS = ('n70_m130', 'n300_m70', 'm1', 'nnz0', 'empty_first_last')


def make_input(name, kind, with_missing):
    """(n, m, indptr, indices, values or None, missing or None): values None = every stored entry is 1; 'f32' / 'f64' hold
    quantitative values with stored zeros and stored NaNs among them; the missing rows include rows that hold entries."""
    n, m, mask = pattern(name)
    indptr, indices = csc_of_mask(mask)
    nnz = indices.shape[0]
    rng = np.random.default_rng(nnz + 7)
    values = None
    if kind != 'ones':
        values = np.round(rng.normal(size=nnz) * 4) / 2
        if nnz >= 4:
            values[rng.choice(nnz, size=max(1, nnz // 9), replace=False)] = 0.0       # stored zeros
            values[rng.choice(nnz, size=max(1, nnz // 11), replace=False)] = np.nan   # stored NaNs
        values = values.astype(np.float32 if kind == 'f32' else np.float64)
    missing = None
    if with_missing:
        missing = np.zeros(n, dtype=np.uint8)
        missing[[0, 7, n // 2, n - 1]] = 1                  # (rows 0 and n - 1 hold entries in most patterns)
    return n, m, indptr, indices, values, missing


def dense_equivalent(n, m, indptr, indices, values, missing, dtype=None):
    if dtype is None:                                       # (no stored value other than 1: the library makes an f32 matrix)
        dtype = np.float32 if values is None or bool((values == 1).all()) else values.dtype
    d = np.zeros((n, m), dtype=dtype, order='F')
    for j in range(m):
        p0, p1 = indptr[j], indptr[j + 1]
        d[indices[p0:p1], j] = 1 if values is None else values[p0:p1]
    if missing is not None:
        d[missing != 0, :] = np.nan
    return d


def sparse_of(n, m, indptr, indices, values, dtype=np.float32):
    data = np.ones(indices.shape[0], dtype=dtype) if values is None else values
    return sp.csc_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(n, m))


def handle_facts(attr, dtype):
    return attr.download(dtype, 'F'), attr.stats(), attr.value_counts(), attr.row_flags()


def assert_same_handle(got, want, what):
    assert got[0].dtype == want[0].dtype, what
    assert np.array_equal(got[0], want[0], equal_nan=True), what
    assert got[1] == want[1], (what, got[1], want[1])
    assert got[2] == want[2], (what, got[2], want[2])
    assert np.array_equal(got[3], want[3]), what


# ------------------------------------------------------------------------------------------------- 1. handle equality ----

@pytest.mark.parametrize('with_missing', [False, True], ids=['all_rows', 'missing_rows'])
@pytest.mark.parametrize('kind', ['ones', 'f32', 'f64'])
@pytest.mark.parametrize('name', PATTERNS)
def test_handle_equals_the_dense_handle(be, ctx, name, kind, with_missing):
    n, m, indptr, indices, values, missing = make_input(name, kind, with_missing)
    dense = dense_equivalent(n, m, indptr, indices, values, missing)
    a = be.Attributes.from_sparse(ctx, sparse_of(n, m, indptr, indices, values), missing_rows=missing)
    d = be.Attributes.from_host(ctx, dense)
    try:
        assert (a.n, a.m, a.dtype) == (n, m, dense.dtype)
        assert_same_handle(handle_facts(a, dense.dtype), handle_facts(d, dense.dtype), (name, kind, with_missing))
    finally:
        a.close()
        d.close()


def test_from_host_dispatches_on_sparse_input(be, ctx):
    n, m, indptr, indices, values, _ = make_input('n70_m130', 'f64', False)
    a = be.Attributes.from_host(ctx, sparse_of(n, m, indptr, indices, values))
    try:
        assert np.array_equal(a.download(np.float64, 'F'), dense_equivalent(n, m, indptr, indices, values, None), equal_nan=True)
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------- 2. result equality ----

def layout(n):
    return np.random.default_rng(100 + n).uniform(size=(n, 2))


def run_safe(amd, n, attribute_file, missing_rows=None, keep=False, sign='highest', **kw):
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(layout(n))
    sf.random_seed = SEED
    sf.attribute_sign = sign
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=RADIUS)
    load = {'attribute_file': attribute_file, 'keep_on_device': keep}
    if missing_rows is not None:
        load['missing_rows'] = missing_rows
    sf.load_attributes(**load)
    sf.compute_pvalues(verbose=False, **kw)
    out = {}
    for key in RESULTS:
        v = getattr(sf, key)
        out[key] = None if v is None else np.array(v)
    out['num_neighborhoods_enriched'] = np.array(sf.attributes['num_neighborhoods_enriched'].values)
    out['kernel'] = sf._ctx().last_kernel()[0]
    return out, sf


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint64 if a.dtype.itemsize == 8 else np.uint8)


def assert_same_results(got, want, what):
    for key in RESULTS + ('num_neighborhoods_enriched',):
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        assert got[key] is not None and got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (what, key)
        assert np.array_equal(bits(got[key]), bits(want[key])), '%s: %s differs from the dense run' % (what, key)


def both_ways(amd, inp, **kw):
    """compute_pvalues on the sparse input and on its dense equivalent (fresh copies: background='network' edits its input)."""
    n, m, indptr, indices, values, missing = inp
    got, sf = run_safe(amd, n, sparse_of(n, m, indptr, indices, values), missing_rows=missing, **kw)
    want, _ = run_safe(amd, n, dense_equivalent(n, m, indptr, indices, values, missing), **kw)
    return got, want, sf


@pytest.mark.parametrize('background', ['attribute_file', 'network'])
def test_binary_hypergeometric(amd, background):
    inp = make_input('n70_m130', 'ones', True)
    got, want, sf = both_ways(amd, inp, how='hypergeometric', background=background)
    assert_same_results(got, want, background)
    assert sp.issparse(sf.node2attribute), 'compute_pvalues densified self.node2attribute'
    assert np.nansum(want['nes_binary']) > 0, 'the case tests nothing: no enriched pair'
    if background == 'network':
        assert sf._missing_rows is None


def binary_without_entries_on_missing_rows(stored_zero):
    """0/1 input whose stored entries ARE the support lists (no entry on a missing row); stored_zero: one explicit zero is
    added, so the lists must come from the dense scan instead."""
    n, m, indptr, indices, _, missing = make_input('n70_m130', 'ones', True)
    mask = np.zeros((n, m), dtype=bool)
    for j in range(m):
        mask[indices[indptr[j]:indptr[j + 1]], j] = True
    mask[missing != 0, :] = False
    zero_at = None
    if stored_zero:
        i, j = np.argwhere(~mask & (missing == 0)[:, None])[17]
        mask[i, j] = True
        zero_at = (i, j)
    indptr, indices = csc_of_mask(mask)
    values = None
    if stored_zero:
        values = np.ones(indices.shape[0], dtype=np.float32)
        k = indptr[zero_at[1]] + int(np.searchsorted(indices[indptr[zero_at[1]]:indptr[zero_at[1] + 1]], zero_at[0]))
        assert indices[k] == zero_at[0]
        values[k] = 0.0
    return n, m, indptr, indices, values, missing


@pytest.mark.parametrize('stored_zero', [False, True], ids=['lists_from_input', 'lists_from_scan'])
@pytest.mark.parametrize('sign', ['highest', 'lowest', 'both'])
def test_binary_randomization_on_the_support_lists(amd, monkeypatch, sign, stored_zero):
    """The scatter form of the permutation test is the consumer of the support lists: forced, so that the lists installed from
    the input (or, with a stored zero, rebuilt by k_fill_support) are what the kernel reads."""
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'scatter')
    inp = binary_without_entries_on_missing_rows(stored_zero)
    got, want, _ = both_ways(amd, inp, sign=sign, how='randomization', num_permutations=NPERM)
    assert got['kernel'] == want['kernel'] == 'k_permtest_scatter', (got['kernel'], want['kernel'])
    assert_same_results(got, want, (sign, stored_zero))
    assert np.nanmin(want['pvalues_pos']) < 1.0


def test_binary_randomization_default_route(amd):
    got, want, _ = both_ways(amd, binary_without_entries_on_missing_rows(False), sign='both', how='randomization', num_permutations=NPERM)
    assert got['kernel'] == want['kernel']
    assert_same_results(got, want, 'default route')


@pytest.mark.parametrize('score', ['sum', 'z-score'])
def test_quantitative_f64(amd, score):
    inp = make_input('n300_m70', 'f64', True)
    got, want, _ = both_ways(amd, inp, how='randomization', num_permutations=NPERM, neighborhood_score_type=score)
    assert got['kernel'] == want['kernel']
    assert_same_results(got, want, score)


def test_multiple_testing(amd):
    got, want, _ = both_ways(amd, make_input('n70_m130', 'ones', True), how='hypergeometric', multiple_testing=True)
    assert_same_results(got, want, 'fdr')


def test_keep_on_device(amd):
    """The resident handle made from the sparse input serves compute_pvalues (no second upload), background='network' included:
    nan_to_zero on the handle, the missing rows cleared on the host side."""
    inp = make_input('n70_m130', 'f32', True)
    n, m, indptr, indices, values, missing = inp
    want, _ = run_safe(amd, n, dense_equivalent(n, m, indptr, indices, values, missing), how='randomization',
                       num_permutations=NPERM, background='network')
    a = sparse_of(n, m, indptr, indices, values)
    got, sf = run_safe(amd, n, a, missing_rows=missing, keep=True, how='randomization', num_permutations=NPERM, background='network')
    assert_same_results(got, want, 'keep_on_device')
    assert sf._resident_attributes() is not None and sf.node2attribute is a
    assert not np.isnan(a.data).any()


# ---------------------------------------------------------------------------------------------------- 3. input forms ----

def test_input_forms_equal_the_csc_result(amd, be, ctx):
    n, m, indptr, indices, _, _ = make_input('n70_m130', 'ones', False)
    base = sparse_of(n, m, indptr, indices, None, dtype=np.float32)
    ref = be.Attributes.from_sparse(ctx, base)
    want_handle = handle_facts(ref, np.float32)
    ref.close()
    want, _ = run_safe(amd, n, base, how='hypergeometric')
    coo = base.tocoo()
    half = sp.coo_matrix((np.concatenate([coo.data, coo.data]) * 0.5, (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))),
                         shape=(n, m))                      # every entry twice, 0.5 + 0.5
    unsorted = base.copy()
    for j in range(m):                                      # row indices of every column reversed: valid scipy, not canonical
        unsorted.indices[indptr[j]:indptr[j + 1]] = unsorted.indices[indptr[j]:indptr[j + 1]][::-1].copy()
    unsorted.has_sorted_indices = False
    i64, i32 = base.copy(), base.copy()                     # (the constructor narrows index arrays: set them afterwards)
    i64.indices, i64.indptr = base.indices.astype(np.int64), base.indptr.astype(np.int64)
    i32.indices, i32.indptr = base.indices.astype(np.int32), base.indptr.astype(np.int32)
    forms = {'csr': base.tocsr(), 'csc': base.copy(), 'coo_duplicates': half, 'int64_indices': i64, 'int32_indices': i32,
             'bool': base.astype(bool), 'int8': base.astype(np.int8), 'float32': base.astype(np.float32), 'unsorted': unsorted,
             'csc_array': sp.csc_array(base)}
    assert i64.indices.dtype == np.int64 and i32.indptr.dtype == np.int32
    for name, a in forms.items():
        before = a.copy()
        h = be.Attributes.from_sparse(ctx, a)
        try:
            assert_same_handle(handle_facts(h, np.float32), want_handle, name)
        finally:
            h.close()
        assert (abs(a - before)).nnz == 0 and type(a) is type(before), '%s: from_sparse changed its input' % name
        got, _ = run_safe(amd, n, a, how='hypergeometric')
        assert_same_results(got, want, name)


# ---------------------------------------------------------------------------------- 4. refusals at the C entry point ----

def raw_create(be, ctx, n, m, indptr, indices, values=None, dtype=0, missing=None, nnz=None):
    from safepy_amd import _lib
    h = C.c_void_p()
    indptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    rc = _lib.lib.safe_attr_create_csc_host(ctx.handle, n, m, indices.shape[0] if nnz is None else nnz,
                                            None if indptr is None else C.c_void_p(indptr.ctypes.data),
                                            C.c_void_p(indices.ctypes.data) if indices.size else None,
                                            None if values is None else C.c_void_p(values.ctypes.data), dtype,
                                            None if missing is None else C.c_void_p(missing.ctypes.data), C.byref(h))
    return rc, h, _lib.lib.safe_last_error().decode()


def test_contract_violations_are_refused(be, ctx):
    """Every broken rule is found by the validation kernel (which reads inside the three arrays only) and refused with
    SAFE_E_VALUE before anything is scattered; no handle, no allocation left behind; the context works afterwards."""
    from safepy_amd import _lib
    n, m = 70, 6
    indptr = np.array([0, 3, 3, 5, 9, 9, 11], dtype=np.int64)
    indices = np.array([0, 4, 69, 2, 3, 0, 1, 50, 69, 10, 68], dtype=np.int32)

    def valid():
        rc, h, msg = raw_create(be, ctx, n, m, indptr, indices)
        assert rc == 0, msg
        a = be.Attributes(ctx, h, n, m)
        got = a.download(np.float32, 'F')
        a.close()
        assert np.array_equal(got, dense_equivalent(n, m, indptr, indices, None, None))

    valid()                                                 # (fills the context's pool: see the module docstring)
    start = be.device_alloc_count()

    def edited(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    cases = {
        'row index == n': (indptr, edited(indices, 2, n), 'outside'),
        'negative row index': (indptr, edited(indices, 5, -1), 'outside'),
        'equal neighbours': (indptr, edited(indices, 6, 0), 'repeated'),
        'descending neighbours': (indptr, edited(indices, 7, 0), 'descend'),
        'indptr decreasing': (edited(indptr, 2, 2), indices, 'indptr decreases'),
        'indptr[m] != nnz': (edited(indptr, m, 10), indices, 'indptr[m]'),
        'indptr[0] != 0': (edited(indptr, 0, 1), indices, 'indptr[0]'),
    }
    for name, (ptr, idx, word) in cases.items():
        rc, h, msg = raw_create(be, ctx, n, m, ptr, idx)
        assert rc == _lib.E_VALUE, (name, rc, msg)
        assert not h.value, name
        assert word in msg, (name, msg)
    rc, h, msg = raw_create(be, ctx, n, m, None, indices)
    assert rc == _lib.E_INVALID and not h.value, (rc, msg)
    valid()
    assert be.device_alloc_count() == start


# ---------------------------------------------------------------------------------------------------- 5. stream order ----

def test_create_behind_a_busy_caller_stream(amd, be, ctx):
    """The create call on a caller's stream that is still busy (tests/test_gpu_stream_order.py: set_stream, a chain of
    kernels queued in front), safe_hypergeom straight behind it without a host synchronisation, outputs snapshotted on the same stream.
    Poison: the outputs hold NaN, and the pool's blocks -- staging, row indices, the dense matrix -- hold the contents of ANOTHER
    matrix of the same sizes, created and destroyed just before; a scatter that ran ahead of its memset or its uploads would
    read or leave them."""
    import torch
    n, m, indptr, indices, _, missing = make_input('n70_m130', 'ones', True)
    dense = dense_equivalent(n, m, indptr, indices, None, missing)
    a = sparse_of(n, m, indptr, indices, None)
    other = sp.csc_matrix((np.ones(indices.shape[0], np.float32), ((indices[::-1] + 13) % n).astype(np.int32), indptr.copy()), shape=(n, m))
    nbr = be.Neighborhoods.euclidean(ctx, layout(n), RADIUS)

    def outputs():
        return [torch.full((n, m), float('nan'), dtype=torch.float64, device='cuda') for _ in range(3)] + \
               [torch.full((m,), float('nan'), dtype=torch.float64, device='cuda')]

    # the dense run, the quiet way
    want = outputs()
    torch.cuda.synchronize()
    d = be.Attributes.from_host(ctx, dense)
    be.hypergeom(ctx, nbr, d, 0.05, [t.data_ptr() for t in want])
    ctx.sync()
    d.close()
    want = [t.cpu().numpy() for t in want]
    # the pool now holds blocks of these sizes with another matrix in them
    be.Attributes.from_sparse(ctx, other, missing_rows=missing).close()

    s = torch.cuda.Stream()
    x = torch.ones(1 << 28, dtype=torch.float32, device='cuda')     # the delay: element-wise passes over 1 GiB, 3 GiB of traffic each
    y = torch.zeros_like(x)
    got, snaps = outputs(), outputs()
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    h = None
    try:
        with torch.cuda.stream(s):
            for _ in range(40):                             # tens of milliseconds: far longer than the create call's own work
                y.add_(x)
            delay_done = torch.cuda.Event()
            delay_done.record(s)
        assert not delay_done.query(), 'the harness drained the busy stream before the call: this would be a quiet run'
        h = be.Attributes.from_sparse(ctx, a, missing_rows=missing)
        be.hypergeom(ctx, nbr, h, 0.05, [t.data_ptr() for t in got])
        with torch.cuda.stream(s):
            for snap, t in zip(snaps, got):
                snap.copy_(t)
                t.fill_(float('nan'))
        s.synchronize()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        if h is not None:
            h.close()
        nbr.close()
    for i, (g, w) in enumerate(zip(snaps, want)):
        assert np.array_equal(bits(g.cpu().numpy()), bits(w)), 'output %d of the busy sparse run differs from the dense run' % i
    assert np.nansum(want[2]) > 0


# --------------------------------------------------------------------------------------------------------- 6. no leak ----

def test_create_destroy_cycles_allocate_nothing(be, ctx):
    inputs = [make_input('n70_m130', 'ones', True), make_input('n70_m130', 'f64', True)]

    def cycle():
        for n, m, indptr, indices, values, missing in inputs:
            a = be.Attributes.from_sparse(ctx, sparse_of(n, m, indptr, indices, values), missing_rows=missing)
            a.stats()
            a.close()

    cycle()                                                 # (fills the context's pool: see the module docstring)
    start = be.device_alloc_count()
    for _ in range(10):
        cycle()
    assert be.device_alloc_count() == start


# --------------------------------------------------------------------------------------------------------- 7. sharding ----

def test_sharded_call_on_a_sparse_column_shard(amd):
    """sharding.sharded_compute_pvalues with a sparse column shard a[:, c0:c1] over a one-rank RCCL group (the collectives
    really run) == the same call with the dense shard, and == the unsplit drop-in call."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from safepy_amd import sharding
    n, m, indptr, indices, values, _ = make_input('n70_m130', 'ones', False)
    a = sparse_of(n, m, indptr, indices, values)
    dense = dense_equivalent(n, m, indptr, indices, values, None)
    want, sf = run_safe(amd, n, dense, how='hypergeometric')
    c0, c1 = sharding.column_shards(m, 1)[0]
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        outs = [sharding.sharded_compute_pvalues(sf._ctx(), sf._device_neighborhoods(), block, m, enrichment_type='hypergeometric',
                                                 gather=('nes', 'nes_binary', 'pvalues_pos'))
                for block in (a[:, c0:c1], np.ascontiguousarray(dense[:, c0:c1]))]
    finally:
        dist.destroy_process_group()
    for key in ('full_nes', 'full_nes_binary', 'full_pvalues_pos', 'num_neighborhoods_enriched'):
        assert np.array_equal(bits(np.asarray(outs[0][key], dtype=np.float64)), bits(np.asarray(outs[1][key], dtype=np.float64))), key
    assert np.array_equal(bits(outs[0]['full_nes']), bits(want['nes']))
    assert np.array_equal(bits(outs[0]['full_nes_binary']), bits(want['nes_binary']))
