"""safe_go_create / read / as_attr (csrc/go.hip) against the networkx restatement (tests/go_ref.py): indptr, indices, the kept
terms and the number of loci given to the root are EQUAL, not close -- the result is a set of bits.

Shapes: row counts around the 32-bit word (31 / 32 / 33), the 64-lane wave step of the emit kernel in words is 2048 loci
(2049), and the 256 words = 8192 loci a workgroup of the level kernel covers (8192 / 8193); term counts 1, 2, 257 (past one
workgroup of the per-term kernels) and 4097 (past one tile of the scan); a 200-level chain, a hub with 5000 children, a term
with 40 parents, random DAGs with 1-3 parents and 12 levels.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import go_ref

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


def run(be, ctx, n_rows, n_terms, edges, ann_row, ann_term, root=0, missing=None):
    ptr, idx = go_ref.children_csr(n_terms, edges)
    g = be.GoClosure(ctx, n_rows, n_terms, ptr, idx, ann_row, ann_term, root, missing)
    try:
        return g.read(), (g.n_kept, g.nnz, g.num_root_assigned)
    finally:
        g.close()


def check(be, ctx, n_rows, n_terms, edges, ann_row, ann_term, root=0, missing=None):
    want = go_ref.closure_ref(n_rows, n_terms, edges, ann_row, ann_term, root, missing)
    (indptr, indices, kept, assigned), (n_kept, nnz, assigned2) = run(be, ctx, n_rows, n_terms, edges, ann_row, ann_term, root, missing)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and kept.dtype == np.int32
    assert (n_kept, nnz) == (want['kept'].shape[0], want['indices'].shape[0])
    assert np.array_equal(kept, want['kept'])
    assert np.array_equal(indptr, want['indptr'])
    assert np.array_equal(indices, want['indices'])
    assert assigned == assigned2 == want['assigned']
    return want


def random_case(seed, n_rows, n_terms, n_levels=12, n_ann=None):
    rng = np.random.default_rng(seed)
    edges = go_ref.random_dag(rng, n_terms, n_levels)
    n_ann = n_ann if n_ann is not None else max(4, min(3 * n_rows, 1500))
    return edges, rng.integers(0, n_rows, n_ann), rng.integers(0, n_terms, n_ann)


@pytest.mark.parametrize('n_rows', [1, 31, 32, 33, 63, 64, 65, 2049, 8192, 8193])
def test_row_counts(be, ctx, n_rows):
    edges, ann_row, ann_term = random_case(n_rows, n_rows, 257, n_ann=min(2 * n_rows + 3, 600))
    ann_row[0] = n_rows - 1                                   # the last locus is always annotated ...
    want = check(be, ctx, n_rows, 257, edges, ann_row, ann_term)
    if n_rows > 64:
        assert want['assigned'] > 0                           # ... and some locus has no term at all


@pytest.mark.parametrize('n_terms', [1, 2, 257, 4097])
def test_term_counts(be, ctx, n_terms):
    edges, ann_row, ann_term = random_case(100 + n_terms, 65, n_terms, n_ann=400)
    check(be, ctx, 65, n_terms, edges, ann_row, ann_term)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_dags(be, ctx, seed):
    edges, ann_row, ann_term = random_case(seed, 700, 900)
    parents = np.bincount([c for _, c in edges], minlength=900)
    assert parents.max() >= 2 and parents[1:].min() >= 1
    check(be, ctx, 700, 900, edges, ann_row, ann_term)


def test_chain_of_200_levels(be, ctx):
    rng = np.random.default_rng(200)
    order = np.concatenate([[0], 1 + rng.permutation(199)])                   # term order[k] is at depth k
    edges = [(int(order[k]), int(order[k + 1])) for k in range(199)]
    ann_row, ann_term = np.arange(100), order[rng.integers(1, 200, 100)]
    ann_term[7] = order[199]                                                  # one locus sits on the deepest term
    want = check(be, ctx, 130, 200, edges, ann_row, ann_term)
    assert want['dense'][7].sum() == 200 and want['assigned'] == 30


def test_hub_with_5000_children(be, ctx):
    rng = np.random.default_rng(5000)
    edges = [(0, 1)] + [(1, c) for c in range(2, 5002)] + [(int(rng.integers(2, 5002)), 5002)]
    ann_row, ann_term = rng.integers(0, 300, 2500), rng.integers(2, 5003, 2500)
    want = check(be, ctx, 300, 5003, edges, ann_row, ann_term)
    assert np.array_equal(want['dense'][:, 0], want['dense'][:, 1])


def test_term_with_40_parents(be, ctx):
    edges = [(0, p) for p in range(1, 41)] + [(p, 41) for p in range(1, 41)] + [(41, 42)]
    want = check(be, ctx, 50, 43, edges, [3, 4, 4], [42, 41, 7])
    assert want['dense'][3].sum() == 43 and want['dense'][4].sum() == 42 and want['assigned'] == 48


@pytest.mark.parametrize('n_rows', [70, 8193])
def test_child_counts_around_the_split_of_the_level_kernel(be, ctx, n_rows):
    """Up to 16 children one wave ORs them alone (8 loads in flight, then a remainder loop); from 17 on the eight waves of the
    workgroup share them: terms with 1 .. 130 children on both sides of 8, 16, 64 (a full round of all waves) and 128."""
    rng = np.random.default_rng(17)
    counts = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 71, 72, 73, 127, 128, 129, 130]
    edges, nxt = [], 1 + len(counts)
    for h, k in enumerate(counts, start=1):
        edges.append((0, h))
        edges.extend((h, c) for c in range(nxt, nxt + k))
        nxt += k
    # a third of the leaves annotated with a locus of their own, so that every child's position matters to its parent
    leaves = np.arange(1 + len(counts), nxt)
    picked = leaves[rng.uniform(size=leaves.size) < 0.34]
    picked = np.union1d(picked, [e[1] for e in edges if e[0] != 0][-1:])              # (the very last child of the last hub too)
    ann_row = rng.integers(0, n_rows - 3, picked.size)
    want = check(be, ctx, n_rows, nxt, edges, ann_row, picked)
    assert want['assigned'] >= 3


# ---------------------------------------------------------------------------------------------------- annotations ----

@pytest.fixture(scope='module')
def dag():
    return go_ref.random_dag(np.random.default_rng(77), 257, 12)


def leaf_of(edges, n_terms):
    return int(np.flatnonzero(np.bincount([p for p, _ in edges], minlength=n_terms) == 0)[-1])


def test_every_annotation_on_one_leaf(be, ctx, dag):
    want = check(be, ctx, 100, 257, dag, np.arange(100), np.full(100, leaf_of(dag, 257)))
    assert want['assigned'] == 0 and set(np.diff(want['indptr']).tolist()) == {100}


def test_duplicate_pairs(be, ctx, dag):
    rng = np.random.default_rng(5)
    r, t = rng.integers(0, 100, 60), rng.integers(0, 257, 60)
    once = check(be, ctx, 100, 257, dag, r, t)
    many = check(be, ctx, 100, 257, dag, np.tile(r, 5), np.tile(t, 5))
    assert np.array_equal(once['indices'], many['indices'])


def test_no_annotation_at_all(be, ctx, dag):
    none = np.empty(0, dtype=np.int32)
    want = check(be, ctx, 100, 257, dag, none, none, root=0)
    assert want['assigned'] == 100 and want['kept'].tolist() == [0] and want['indices'].tolist() == list(range(100))


def test_annotations_on_the_root_only(be, ctx, dag):
    want = check(be, ctx, 100, 257, dag, [5, 9, 5], [0, 0, 0])
    assert want['assigned'] == 98 and want['kept'].tolist() == [0] and want['indptr'].tolist() == [0, 100]


def test_all_rows_missing(be, ctx, dag):
    none = np.empty(0, dtype=np.int32)
    ptr, idx = go_ref.children_csr(257, dag)
    want = check(be, ctx, 100, 257, dag, none, none, missing=np.ones(100, dtype=np.uint8))
    assert want['assigned'] == 0 and want['kept'].size == 0 and want['indptr'].tolist() == [0]
    g = be.GoClosure(ctx, 100, 257, ptr, idx, none, none, 0, np.ones(100, dtype=np.uint8))
    with pytest.raises(be._lib.SafeHipError) as err:                          # no term is left: there is no matrix
        g.as_attributes()
    assert err.value.code == be._lib.E_INVALID
    g.close()


def test_some_rows_missing(be, ctx, dag):
    rng = np.random.default_rng(8)
    missing = (rng.uniform(size=100) < 0.3).astype(np.uint8)
    live = np.flatnonzero(missing == 0)
    r, t = live[rng.integers(0, live.size - 10, 40)], rng.integers(0, 257, 40)   # the last ten live loci have no term
    want = check(be, ctx, 100, 257, dag, r, t, missing=missing)
    assert want['assigned'] >= 10 and not want['dense'][missing != 0].any()


def test_file_order_decides_between_two_parentless_terms(be, ctx):
    """Terms B < A < C < I by id; A -> C, B -> C; I stands alone.  The first parentless term of the FILE takes the loci
    without a term, whatever its place among the sorted columns."""
    from safepy_amd.utils import make_go
    import pandas as pd
    ids = {'A': 'GO:0000002', 'B': 'GO:0000001', 'C': 'GO:0000003', 'I': 'GO:0000004'}
    ns = {t: 'biological_process' for t in ids.values()}
    ann = pd.DataFrame({1: ['x', 'y', 'z'], 4: [ids['C'], 'GO:0999999', 'GO:0999999']})
    for first, root in (('I', ids['I']), ('A', ids['A']), ('B', ids['B'])):
        rest = [k for k in 'CABI' if k != first]
        g = make_go.GoGraph([ids[first]] + [ids[k] for k in rest], ns, {t: t for t in ns}, [(ids['A'], ids['C']), (ids['B'], ids['C'])], set(ns))
        gm = make_go.make_locus2term(g, ann)
        ref = go_ref.matrix_ref(g, [('x', ids['C']), ('y', 'GO:0999999'), ('z', 'GO:0999999')], 'p')
        assert gm.root == ref['root'] == root and gm.terms == ref['terms'] and gm.num_root_assigned == 2
        assert np.array_equal(gm.matrix.toarray(), ref['ints'])
        assert gm.matrix.toarray()[:, gm.terms.index(root)].tolist() == ([1, 1, 1] if first != 'I' else [0, 1, 1])
        gm.release()


# ------------------------------------------------------------------------------------------------ device behaviour ----

def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('with_missing', [False, True])
def test_as_attributes_equals_from_sparse_of_the_read_csc(be, ctx, dag, with_missing):
    rng = np.random.default_rng(11)
    n_rows = 333
    missing = (rng.uniform(size=n_rows) < 0.2).astype(np.uint8) if with_missing else None
    live = np.flatnonzero(missing == 0) if with_missing else np.arange(n_rows)
    r, t = live[rng.integers(0, live.size, 500)], rng.integers(0, 257, 500)
    ptr, idx = go_ref.children_csr(257, dag)
    g = be.GoClosure(ctx, n_rows, 257, ptr, idx, r, t, 0, missing)
    indptr, indices, kept, _ = g.read()
    on_device = g.as_attributes()
    g.close()                                                 # the matrix does not need the handle any more
    got = on_device.download(np.float32, order='F')
    on_device.close()
    m = sp.csc_array((np.ones(indices.size, dtype=np.float32), indices, indptr), shape=(n_rows, kept.size))
    via_host = be.Attributes.from_sparse(ctx, m, missing)
    want = via_host.download(np.float32, order='F')
    via_host.close()
    assert got.shape == want.shape == (n_rows, kept.size)
    assert np.array_equal(f32_bits(got), f32_bits(want))
    ref = go_ref.closure_ref(n_rows, 257, dag, r, t, 0, missing)
    dense = ref['dense'][:, ref['kept']].astype(np.float32)
    if with_missing:
        dense[missing != 0] = np.nan
        assert np.isnan(got[missing != 0]).all()
    assert np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(dense, nan=-1.0))


def test_same_call_twice_same_bytes(be, ctx):
    edges, r, t = random_case(21, 2049, 900)
    first, _ = run(be, ctx, 2049, 900, edges, r, t)
    second, _ = run(be, ctx, 2049, 900, edges, r, t)
    for a, b in zip(first[:3], second[:3]):
        assert a.tobytes() == b.tobytes()
    assert first[3] == second[3]


def test_on_a_busy_caller_stream(be, ctx):
    """The context switched to a caller's stream that is busy with a chain of matrix products when the call arrives: the call
    queues behind it, waits for its own totals, and gives the bytes of the quiet run; as_attributes behind it too."""
    import torch
    edges, r, t = random_case(31, 700, 900)
    ptr, idx = go_ref.children_csr(900, edges)

    def once():
        g = be.GoClosure(ctx, 700, 900, ptr, idx, r, t, 0, None)
        attr = g.as_attributes()
        out = g.read()[:3] + (attr.download(np.float32, order='F'),)
        attr.close()
        g.close()
        return out
    quiet = once()
    s = torch.cuda.Stream()
    a = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device='cuda')
    c = torch.empty_like(a)
    torch.cuda.synchronize()
    ctx.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            for _ in range(40):
                torch.mm(a, a, out=c)
            done = torch.cuda.Event()
            done.record(s)
        assert not done.query(), 'the delay had drained before the call: the stream was not busy'
        busy = once()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
    for q, b in zip(quiet, busy):
        assert q.tobytes() == b.tobytes()


def test_live_allocations_are_steady(be, ctx):
    edges, r, t = random_case(41, 333, 257)
    ptr, idx = go_ref.children_csr(257, edges)
    missing = np.zeros(333, dtype=np.uint8)
    missing[5] = 1
    r = np.where(r == 5, 6, r)

    def pair():
        g = be.GoClosure(ctx, 333, 257, ptr, idx, r, t, 0, missing)
        g.read()
        g.close()
    pair()                                                    # the context's scratch grows once
    before = be.device_live_alloc_count()
    for _ in range(20):
        pair()
    assert be.device_live_alloc_count() == before


def raw_create(be, ctx, n_rows, n_terms, ptr, idx, r, t, root, missing=None, n_ann=None):
    """The C call itself with sentinels behind every output pointer: (return code, outputs as left)."""
    h = C.c_void_p(0xDEAD)
    n_kept, nnz, assigned, ms = C.c_int64(-7), C.c_int64(-8), C.c_int64(-9), C.c_double(-1.5)
    ptr, idx = np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32)
    r, t = np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(t, dtype=np.int32)
    rc = be.lib.safe_go_create(ctx.handle, n_rows, n_terms, be._ptr(ptr), be._ptr(idx) if idx.size else None,
                               r.size if n_ann is None else n_ann, be._ptr(r) if r.size else None, be._ptr(t) if t.size else None, root,
                               be._ptr(missing), C.byref(h), C.byref(n_kept), C.byref(nnz), C.byref(assigned), C.byref(ms))
    return rc, (h.value, n_kept.value, nnz.value, assigned.value, ms.value)


def test_refusals_return_their_code_and_touch_no_output(be, ctx):
    E_VALUE = be._lib.E_VALUE
    untouched = (0xDEAD, -7, -8, -9, -1.5)
    ptr, idx = go_ref.children_csr(4, [(0, 1), (1, 2), (2, 3)])
    before = be.device_live_alloc_count()
    cases = {
        'cycle': lambda: raw_create(be, ctx, 5, 4, *go_ref.children_csr(4, [(0, 1), (1, 2), (2, 3), (3, 1)]), [0], [1], 0),
        'self loop': lambda: raw_create(be, ctx, 5, 4, *go_ref.children_csr(4, [(0, 1), (2, 2)]), [0], [1], 0),
        'child index out of range': lambda: raw_create(be, ctx, 5, 4, ptr, np.array([1, 2, 4]), [0], [1], 0),
        'negative child index': lambda: raw_create(be, ctx, 5, 4, ptr, np.array([1, -1, 3]), [0], [1], 0),
        'annotation row out of range': lambda: raw_create(be, ctx, 5, 4, ptr, idx, [5], [1], 0),
        'annotation term out of range': lambda: raw_create(be, ctx, 5, 4, ptr, idx, [0], [4], 0),
        'negative annotation row': lambda: raw_create(be, ctx, 5, 4, ptr, idx, [-1], [1], 0),
        'root out of range': lambda: raw_create(be, ctx, 5, 4, ptr, idx, [0], [1], 4),
        'annotation on a missing row': lambda: raw_create(be, ctx, 5, 4, ptr, idx, [2], [1], 0, np.array([0, 0, 1, 0, 0], dtype=np.uint8)),
        'n_rows past int32': lambda: raw_create(be, ctx, 1 << 31, 4, ptr, idx, [0], [1], 0),
        'n_terms past int32': lambda: raw_create(be, ctx, 5, 1 << 31, ptr, idx, [0], [1], 0),
        'annotation count past int32': lambda: raw_create(be, ctx, 5, 4, ptr, idx, [0], [1], 0, n_ann=1 << 31),
        'no rows': lambda: raw_create(be, ctx, 0, 4, ptr, idx, [], [], 0),
    }
    for name, call in cases.items():
        rc, outputs = call()
        assert rc == E_VALUE, (name, rc, be.lib.safe_last_error())
        assert outputs == untouched, name
        assert be.lib.safe_last_error().startswith(b'safe_go_create'), name
    assert be.device_live_alloc_count() == before             # refused before anything was allocated
    rc, outputs = raw_create(be, ctx, 5, 4, ptr, idx, [0], [3], 0)            # (the same inputs, valid: the sentinels go)
    assert rc == 0 and outputs[1:4] == (4, 8, 4)
    be.check(be.lib.safe_go_destroy(C.c_void_p(outputs[0])))
    with pytest.raises(be._lib.SafeHipError) as err:
        be.GoClosure(ctx, 5, 4, *go_ref.children_csr(4, [(0, 1), (1, 0)]), [0], [1], 0)
    assert err.value.code == E_VALUE and 'cycle' in str(err.value)


def test_pass_times_and_levels(be, ctx):
    edges, r, t = random_case(51, 8193, 4097, n_ann=1500)
    ptr, idx = go_ref.children_csr(4097, edges)
    g = be.GoClosure(ctx, 8193, 4097, ptr, idx, r, t, 0, None)
    ms, levels = g.pass_ms()
    g.close()
    assert levels == 12 and set(ms) == set(be.GoClosure.PASSES) and all(v >= 0 for v in ms.values())
    assert abs(sum(ms.values()) - g.kernel_ms) < 1e-6
