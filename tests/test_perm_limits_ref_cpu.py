"""tests/perm_limits_ref.py without a GPU: its limits against the byte formulas and constants read out of
safepy_amd/csrc/enrich.hip (a change of a kernel's LDS footprint fails here first), its counters and outputs against the oracle's
own loop bit for bit, and the tolerance cap of the z-score cases of tests/test_gpu_perm_limits.py established on the reference
alone: on every z-score input of that file no permutation lies within the band of 1e-9 around the observed score, so the
counters the device must give are exactly the reference's."""
import os
import re

import numpy as np
import pytest

import perm_limits_ref as plr
from oracle import safe_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'safepy_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def squeezed(text):
    """Without any whitespace: a reformat of the source changes nothing here."""
    return re.sub(r'\s+', '', text)


def count(code, snippet):
    return squeezed(code).count(squeezed(snippet))


def c_function(code, name, args):
    """The one return expression of `static size_t name(args)` as a Python function of the same arguments."""
    found = re.search(r'static\s+size_t\s+%s\s*\(([^)]*)\)\s*\{\s*return\b([^;]*);\s*\}' % name, code)
    assert found, name
    assert [a.split()[-1] for a in found.group(1).split(',')] == args, found.group(1)
    expr = found.group(2)
    expr = re.sub(r'static_cast\s*<\s*size_t\s*>', '', expr)
    expr = re.sub(r'sizeof\s*\(\s*unsigned\s+int\s*\)', '4', expr)
    expr = re.sub(r'sizeof\s*\(\s*unsigned\s+short\s*\)', '2', expr)
    expr = re.sub(r'size_t\s*\(\s*1\s*\)', '1', expr)
    assert re.fullmatch(r'[\s0-9()+*&~a-z_]*', expr) and set(re.findall(r'[a-z_][a-z_0-9]*', expr)) <= set(args), expr
    return lambda *values: eval(expr, {'__builtins__': {}}, dict(zip(args, values)))     # (an arithmetic expression of the arguments)


def largest_within(fits):
    n = 1
    while fits(n + 1):
        n += 1
    return n


# ------------------------------------------------------------------------------------------------- the constants ----

def test_the_limits_are_the_ones_the_source_derives():
    code, rng = source('enrich.hip'), source('rng.cpp')
    lds = c_function(code, 'ldsf64_bytes', ['n', 'stride16'])
    scatter = c_function(code, 'scatter_lds_bytes', ['n'])
    # stride16 of a table handle, and the budget both routes compare with
    assert count(rng, 'p->stride16 = (stride + 7) / 8 * 8;') >= 1 and count(rng, 'stride = n + 1') >= 1
    assert count(rng, 'p->stride16 =') == count(rng, 'p->stride16 = (stride + 7) / 8 * 8;')      # (no other rule anywhere)
    assert count(code, 'ldsf64_bytes(nbr->n, perms->stride16) <= 160 * 1024') == 1
    assert count(code, 'nbr->max_count < SC_EPOCH && scatter_lds_bytes(nbr->n) <= 160 * 1024') == 1
    assert plr.LDS_BUDGET == 160 * 1024 == 163840
    stride16 = lambda n: (n + 1 + 7) // 8 * 8
    for n in (1, 2, 7, 8, 9, 4549, 4550, 16382, 16383):
        assert lds(n, stride16(n)) == plr.lds_f64_bytes(n) and scatter(n) == plr.scatter_bytes(n), n
    assert plr.LDS_F64_MAX_N == largest_within(lambda n: lds(n, stride16(n)) <= plr.LDS_BUDGET) == 4549
    assert plr.SCATTER_MAX_N == largest_within(lambda n: scatter(n) <= plr.LDS_BUDGET) == 16382
    assert (plr.lds_f64_bytes(4549), plr.lds_f64_bytes(4550)) == (163824, 163856)
    assert (plr.scatter_bytes(16382), plr.scatter_bytes(16383)) == (163836, 163848)
    epoch = int(re.search(r'#define\s+SC_EPOCH\s+(\d+)u', code).group(1))
    assert plr.SCATTER_MAX_MEMBERS == epoch - 1 == 4095
    assert int(re.search(r'#define\s+SC_CHUNK\s+(\d+)\b', code).group(1)) == 16
    # the packed counters: both routes end at P = 65 535
    assert count(code, 'perms->count >= 1 && perms->count <= %d && ldsf64_bytes' % plr.PACKED_MAX_P) == 1
    assert count(code, 'if (!z && n_perm >= 1 && n_perm <= %d && safe_attr_prepare' % plr.PACKED_MAX_P) == 1
    assert plr.PACKED_MAX_P == 2 ** 16 - 1
    # the prefetch of the scatter kernel reads two chunks past the current one: the padding of the transposed inverse table
    assert count(rng, 'perms->inv_stride = ((perms->count + 15) / 16) * 16 + 32;') == 1


def test_the_small_shapes_lie_on_both_sides_of_every_step():
    stride16 = [8 * ((n + 8) // 8) for n in plr.SMALL_NS]
    assert stride16[:5] == [8, 8, 8, 16, 16]                            # N + 1 on both sides of 8
    slices = [-(-n // 64) for n in plr.SMALL_NS]
    assert slices[5:] == [1, 1, 2, 16, 16, 17]                           # one slice (fifteen idle waves); 16 / 17: a second workgroup
    assert all(plr.lds_f64_bytes(n) <= plr.LDS_BUDGET for n in plr.SMALL_NS)
    assert max(plr.SMALL_NS) + 1 <= 8192                                 # (vec_per_row = stride16 / 8 never exceeds the 1024 threads)
    for n in plr.SMALL_NS:                                              # (a block of nothing but 0 and 1 would leave for the integer forms)
        for m in (1, 3, 4, 5):
            v = plr.small_case(n, 'sum', m)[2]
            assert v.shape == (n, m) and not np.isin(v[~np.isnan(v)], [0.0, 1.0]).all(), (n, m)
    assert plr.radius_for(300) == 0.12 and plr.radius_for(4549) == 0.04 and plr.radius_for(16382) == 0.012


# ------------------------------------------------------------------------------------ the reference is the oracle's ----

N0, P0, SEED0 = 120, 25, 5


@pytest.fixture(scope='module')
def dense_case():
    xy = plr.layout(N0, 3)
    a = orc.neighborhoods_euclidean(xy, 0.15)
    a[7] = 0                                                             # an empty neighborhood
    A = plr.membership_csr(*plr.csr_of_dense(a), N0)
    assert np.array_equal(A.toarray(), a)
    return a, A


def same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), what


@pytest.mark.parametrize('kind', ['dyadic', 'binary'])
def test_sum_counters_and_outputs_are_the_oracles(dense_case, kind):
    a, A = dense_case
    b = plr.dyadic(N0, 4, 8) if kind == 'dyadic' else plr.binary(N0, 4, 8, [0.5, 0.05, 1.0, 0.0])
    tables = orc.permutation_index_table(b, P0, SEED0)
    ns, neg, pos = plr.counts_sum(A, b, tables)
    want_neg, want_pos = orc.run_permutations(a, b.copy(), 'sum', P0, SEED0)
    same(ns, orc.compute_neighborhood_score(a, b, 'sum'), 'ns')
    same(neg, want_neg, 'neg')
    same(pos, want_pos, 'pos')
    assert (neg != P0).any() and (pos != P0).any()
    bn, bneg, bpos = plr.counts_sum_batched(a, b, tables)
    same(bn, ns, 'batched ns'), same(bneg, neg, 'batched neg'), same(bpos, pos, 'batched pos')
    for sign in ('both', 'highest', 'lowest'):
        r = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', neighborhood_score_type='sum', num_permutations=P0,
                                random_seed=SEED0, attribute_sign=sign, enrichment_threshold=0.05)
        got = plr.outputs(ns, neg, pos, P0, sign, 0.05)
        for key in got:
            same(got[key], r[key], '%s %s' % (sign, key))
        assert r['nes_binary'].any()


def test_sum_refuses_values_off_the_grid(dense_case):
    _, A = dense_case
    b = plr.dyadic(N0, 2, 8)
    b[0, 0] = 0.1
    with pytest.raises(AssertionError):
        plr.counts_sum(A, b, np.arange(N0)[None])
    b[0, 0] = 2.0 ** 53
    with pytest.raises(AssertionError):
        plr.counts_sum(A, b, np.arange(N0)[None])


def test_z_counters_and_outputs_are_the_oracles(dense_case):
    a, A = dense_case
    b = plr.normal(N0, 4, 9)
    tables = orc.permutation_index_table(b, P0, SEED0)
    ns, neg, pos, unclear = plr.counts_z(A, b, tables)
    assert unclear.sum() == 0
    want_ns = orc.compute_neighborhood_score(a, b, 'z-score')
    assert np.isnan(want_ns).any() and not np.isnan(want_ns).all()
    np.testing.assert_allclose(ns, want_ns, rtol=1e-12, atol=1e-12, equal_nan=True)
    want_neg, want_pos = orc.run_permutations(a, b.copy(), 'z-score', P0, SEED0)
    ok = unclear == 0
    assert np.array_equal(neg[ok], want_neg[ok]) and np.array_equal(pos[ok], want_pos[ok])
    r = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', neighborhood_score_type='z-score', num_permutations=P0,
                            random_seed=SEED0, attribute_sign='both', enrichment_threshold=0.05)
    got = plr.outputs(want_ns, neg, pos, P0, 'both', 0.05)
    for key in got:
        same(got[key], r[key], key)


def test_a_tie_is_tallied_and_not_counted():
    """An identity row ties every cell with a score: unclear, counted on neither side; NaN scores are clear and count nowhere."""
    A = plr.membership_csr(*plr.csr_of_dense(plr.small_membership(9)), 9)
    b = plr.normal(9, 2, 1)
    b[:] = np.where(np.isnan(b), 0.25, b)
    ns, neg, pos, unclear = plr.counts_z(A, b, plr.rotation_table(9, 3, 0))
    scored = ~np.isnan(ns)
    assert scored.any() and np.isnan(ns[1]).all()
    assert np.array_equal(unclear, 3.0 * scored) and not neg.any() and not pos.any()


# --------------------------------------------------------------------------------------------- the tolerance cap ----

def z_reference(n, m, n_perm, values, indptr, indices):
    A = plr.membership_csr(indptr, indices, n)
    tables = orc.permutation_index_table(values, n_perm, plr.PERM_SEED)
    return plr.counts_z(A, values, tables), np.diff(indptr)


@pytest.mark.parametrize('case', sorted(plr.Z_LIMIT_CASES))
def test_no_permutation_is_unclear_at_the_limit_shapes(case):
    n, m, n_perm, r, layout_seed, value_seed = plr.Z_LIMIT_CASES[case]
    assert r == plr.radius_for(n)
    values = plr.normal(n, m, value_seed)
    (ns, neg, pos, unclear), members = z_reference(n, m, n_perm, values, *plr.euclidean_csr(plr.layout(n, layout_seed), r))
    print('%s: %d unclear of %d cell-permutations, %d NaN scores of %d, %d .. %d members' %
          (case, unclear.sum(), ns.size * n_perm, np.isnan(ns).sum(), ns.size, members.min(), members.max()))
    assert unclear.sum() == 0
    assert np.isnan(ns).mean() < 0.01
    assert (neg != n_perm).any() and (pos != n_perm).any() and (neg + pos <= n_perm).all()    # (no tie: never both)


@pytest.mark.parametrize('n', plr.SMALL_NS)
def test_no_permutation_is_unclear_at_the_small_shapes(n):
    """(A neighborhood below three members with a value has no z-score, so the small networks are mostly NaN: that is their
    point.  The share is bounded only at the limit shapes above.)  On 7, 8 and 9 nodes the fixed matrices of
    perm_limits_ref.small_membership_z keep scored neighborhoods -- at least three per column -- whose counters move."""
    for m in (1, 2):
        a, xy, values = plr.small_case(n, 'z-score', m)
        if a is not None:
            assert np.array_equal(a, plr.small_membership_z(n)) and a.diagonal()[np.arange(n) != 1].all() and (n < 2 or not a[1].any())
        csr = plr.csr_of_dense(a) if a is not None else plr.euclidean_csr(xy, plr.SMALL_RADIUS)
        (ns, neg, pos, unclear), _ = z_reference(n, m, plr.SMALL_PERMS, values, *csr)
        assert unclear.sum() == 0, (n, m)
        if n >= 7:
            assert (~np.isnan(ns)).sum(axis=0).min() >= 3, (n, m)
            assert (neg != plr.SMALL_PERMS).any() and (pos != plr.SMALL_PERMS).any() and neg.any() and pos.any(), (n, m)
        if n >= 1023:
            assert np.isnan(ns).mean() < 0.01


# ---------------------------------------------------------------------------------------------------- the inputs ----

def test_the_builders_are_seeded_and_shaped_as_the_cases_need():
    for build in (lambda: plr.layout(50, 2), lambda: plr.dyadic(60, 3, 2), lambda: plr.normal(60, 3, 2),
                  lambda: plr.binary(60, 3, 2, [0.1, 0.9]), lambda: plr.binary_supports(60, [0, 1, 59, 60, None], 2)):
        assert np.array_equal(build(), build(), equal_nan=True)
    q = plr.dyadic(200, 3, 4)
    assert np.isnan(q).all(axis=1).sum() >= 200 // 25 and 0 < np.isnan(q).mean() < 0.1
    assert np.array_equal(np.nan_to_num(q) * 16, np.round(np.nan_to_num(q) * 16))
    b = plr.binary_supports(300, [0, 1, 64, 255, 256, 257, 300, None], 5)
    assert b.sum(axis=0)[:7].tolist() == [0, 1, 64, 255, 256, 257, 300] and set(np.unique(b)) == {0.0, 1.0}
    d = plr.binary(400, 6, 6, [1.0, 0.99, 0.3, 0.01, 0.0], nan_rows=False)
    assert not np.isnan(d).any() and d[:, 0].all() and not d[:, 4].any()
    for n in (1, 2, 7, 8, 9, 12):
        a = plr.small_membership(n)
        assert a.shape == (n, n) and (n < 2 or not a[1].any()) and (n < 3 or a[n - 1].all())
    assert plr.rotation_table(5, 2, 1).tolist() == [[1, 2, 3, 4, 0]] * 2


@pytest.mark.parametrize('biggest', [plr.SCATTER_MAX_MEMBERS, plr.SCATTER_MAX_MEMBERS + 1])
def test_hub_membership(biggest):
    a = plr.hub_membership(4200, biggest, 9)
    sizes = a.sum(axis=1)
    assert a.dtype == np.int64 and sizes[0] == biggest == sizes.max() and sizes[1] == biggest - 1
    assert (sizes >= 2048).sum() == 6 and sizes[6] == 0 and sizes[7:].max() < 40 and sizes[7:].min() >= 1
    assert set(np.unique(a)) == {0, 1}


def test_every_permutation_of_the_sweep_moves_some_counter():
    """The P sweep of the scatter kernel's prefetch queue: a kernel that took a stale or a wrong queue entry for ONE permutation
    would use another row of the table (or the identity) there.  Every row of the sweep's longest table differs from the
    identity and from each of its neighbours in some cell's compare, so such a slip changes a counter.  (The seeded table of
    P permutations is the first P rows of a longer one: the stream is cumulative.)"""
    n = 300
    values = plr.binary_supports(n, plr.SWEEP_SUPPORTS, plr.SWEEP_SEED)
    A = plr.membership_csr(*plr.euclidean_csr(plr.layout(n, n), plr.radius_for(n)), n)
    tables = orc.permutation_index_table(values, max(plr.SWEEP_PERMS), plr.PERM_SEED)
    assert np.array_equal(tables[:17], orc.permutation_index_table(values, 17, plr.PERM_SEED))
    ns = np.asarray(A @ values)
    le = np.stack([np.asarray(A @ values[t]) <= ns for t in tables])
    ge = np.stack([np.asarray(A @ values[t]) >= ns for t in tables])
    assert all(not (le[p] & ge[p]).all() for p in range(len(tables)))
    for d in (1, 2, 16, 32):                                             # the next entry, the next chunk, the chunk after
        assert all((le[p] != le[p + d]).any() or (ge[p] != ge[p + d]).any() for p in range(len(tables) - d)), d
    assert plr.SWEEP_PERMS == (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)
    assert values.sum(axis=0)[:7].tolist() == [0, 1, 64, 255, 256, 257, 300]


def test_the_saturated_reference_really_saturates():
    a, bits, quant = plr.saturation_inputs()
    assert not a[1].any() and a[plr.SATURATION_N - 1].all()
    for b in (bits, quant):
        tables = orc.permutation_index_table(b, plr.PACKED_MAX_P, plr.PERM_SEED)
        ns, neg, pos = plr.counts_sum_batched(a, b, tables)
        assert ((neg == plr.PACKED_MAX_P) & (pos == plr.PACKED_MAX_P)).sum() >= plr.SATURATION_N
        assert (neg[:, 1] == plr.PACKED_MAX_P).all() and (pos[:, 1] == plr.PACKED_MAX_P).all()
        assert (neg < plr.PACKED_MAX_P).any() and (pos < plr.PACKED_MAX_P).any() and (ns != 0).any()
