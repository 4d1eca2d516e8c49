"""Every launch plan that is sized from the chip's CU count, run where a workgroup serves several units of work.

On 256 CUs the small shapes of the suite give every plan more workgroups than work, so the body of a stride loop or of a
queue loop runs at most once per workgroup: state carried over passes, LDS put back between two attributes, barriers that
idle waves keep reaching and the partly filled last stride never run.  Here the contexts are created with
SAFE_HIP_PLAN_CUS = 1 and 2 (the planning CU count), beside the process-wide context on the whole chip.
tests/plan_ref.py restates the plans and holds the shapes; tests/test_plan_ref_cpu.py shows on the CPU that each shape makes a
second pass at 1 and 2 CUs and a single one at 256.

Every case checks its outputs on every context against the existing plain reference (weights_ref, maxt_ref, the oracle's
score loop, radius_ref, nearest_ref, shortpath_ref, prep_ref), exactly, and the contexts against each other byte for byte.
The values lie on a dyadic grid (multiples of 1/16), so sums are exact in any order: no tolerance appears in this file.
Outputs go into poisoned buffers with a guard band (test_gpu_maxt.Poisoned): a skipped unit shows as poison.

No result may depend on the planning CU count: that is the contract these tests pin.  Needs an MI355X."""
import os

import numpy as np
import pytest

import maxt_ref as mx
import nearest_ref as nrf
import plan_ref as pl
import prep_ref as pr
import radius_ref as rr
import shortpath_ref as sr
import test_gpu_maxt as tm
import test_gpu_prep_edges as tp
import test_gpu_routes as tr
import test_gpu_shortpath as ts
import weights_ref as wr
from oracle import safe_oracle as orc            # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu

VAR = 'SAFE_HIP_PLAN_CUS'
SEED = 11
F64, U8 = np.float64, np.uint8


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def be(amd):
    from safepy_amd import backend
    return backend


def context_with(be, value):
    """A fresh context created while SAFE_HIP_PLAN_CUS is `value` (None: unset); the environment is put back."""
    saved = os.environ.get(VAR)
    try:
        if value is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = value
        return be.Context(0)
    finally:
        if saved is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = saved


@pytest.fixture(scope='module')
def plans(be):
    """{planning CU count: context}: 1, 2 and the process-wide context (the device's own count).  The small contexts live to the
    end of the process, like the default one: handles that outlive a test may still name them."""
    full = be.Context.default(0)
    assert full.num_cu > max(pl.SMALL_CUS), 'the default context is not on the whole chip: is %s set for the whole run?' % VAR
    out = {}
    for k in pl.SMALL_CUS:
        out[k] = context_with(be, str(k))
        assert out[k].num_cu == k
    out[full.num_cu] = full
    yield out
    for k in pl.SMALL_CUS:
        out[k].sync()
        out[k].trim()


class _Once:
    def __init__(self):
        self.memo = {}

    def __call__(self, key, build):
        if key not in self.memo:
            self.memo[key] = build()
        return self.memo[key]


once = _Once()                                                          # references: built on first use, shared, never changed


def same(got, want, what):
    """Equal shapes, NaN in the same cells, equal f64 bits (or integers) everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype.kind != 'f':
        assert np.array_equal(got, want), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ': NaN cells'
    bad = np.argwhere((tm.bits(got) != tm.bits(want.astype(F64))) & ~nan)
    assert bad.shape[0] == 0, (what, '%d cells differ, first at' % bad.shape[0], bad[:4].tolist())


def check_plans(outs, want, what):
    """outs: {CU count: {name: array}}.  Each against `want` (the names it holds), and all of them byte for byte against the first."""
    first_k = next(iter(outs))
    for k, out in outs.items():
        for name, ref in want.items():
            same(out[name], ref, '%s, %d CUs, %s' % (what, k, name))
        for name, arr in out.items():
            other = outs[first_k][name]
            assert arr.dtype == other.dtype and arr.tobytes() == other.tobytes(), '%s: %s at %d CUs is not what %d CUs gave' % (what, name, k, first_k)


def assert_plan(case, plans):
    """The contexts really are in the regime plan_ref promises: a second pass on the small ones, one pass on the whole chip."""
    _, cus, passes = pl.gpu_cases()[case]
    for k, ctx in plans.items():
        assert (passes(ctx.num_cu).most >= 2) == (k in cus), (case, k, passes(ctx.num_cu))


def dyadic(rng, shape, scale=1.0):
    return np.round(rng.normal(size=shape) * scale * 16) / 16


def quantitative(n, m, seed):
    """Multiples of 1/16 with NaN cells and rows without a value."""
    rng = np.random.default_rng(seed)
    b = dyadic(rng, (n, m))
    b[rng.uniform(size=b.shape) < 0.03] = np.nan
    b[rng.choice(n, n // 25, replace=False)] = np.nan
    return b


def run_enrichment(be, ctx, a, b, score, n_perm, entries, kernel, order='C'):
    """permtest_counts / randomization / score of one input on one context into poisoned buffers: {output name: array}."""
    n, m = b.shape
    nbr = be.Neighborhoods.from_dense(ctx, a)
    attr = be.Attributes.from_host(ctx, np.asarray(b, order=order))
    perms = be.Permutations(ctx, n, attr.row_flags(), n_perm, SEED)
    cell = ((n, m), F64)
    shapes = {'counts': {'c_ns': cell, 'c_neg': cell, 'c_pos': cell},
              'randomization': {'r_ns': cell, 'r_pn': cell, 'r_pp': cell, 'r_nes': cell, 'r_nb': cell, 'r_enriched': ((m,), F64)},
              'score': {'s_ns': cell}}
    out = tm.Poisoned(ctx, {name: s for e in entries for name, s in shapes[e].items()})
    try:
        if 'counts' in entries:
            be.permtest_counts(ctx, nbr, attr, perms, score, out.ptr('c_ns'), out.ptr('c_neg'), out.ptr('c_pos'))
            assert ctx.last_kernel()[0] == kernel, ctx.last_kernel()[0]
        if 'randomization' in entries:
            be.randomization(ctx, nbr, attr, perms, score, 'both', 0.05, [out.ptr(k) for k in shapes['randomization']])
            assert ctx.last_kernel()[0] == kernel, ctx.last_kernel()[0]
        if 'score' in entries:
            be.score(ctx, nbr, attr, score, out.ptr('s_ns'))
        got = {name: out.read(name) for name in out.shapes}
        got['tables'] = perms.read()
        return got
    finally:
        out.free()
        perms.close()
        attr.close()
        nbr.close()


def enrichment_reference(a, b, score, n_perm, entries):
    """The oracle's loop (oracle/safe_oracle.py: compute_neighborhood_score per permuted matrix) on the seeded stream."""
    want = {}
    ns = orc.compute_neighborhood_score(a, b, score)
    if 'counts' in entries:
        neg, pos = orc.run_permutations(a, b.copy(), score, n_perm, SEED)
        want.update({'c_ns': ns, 'c_neg': neg, 'c_pos': pos})
    if 'randomization' in entries:
        r = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', neighborhood_score_type=score, num_permutations=n_perm,
                                random_seed=SEED, attribute_sign='both', enrichment_threshold=0.05)
        assert r['nes_binary'].any(), 'no enriched cell: the fused epilogue would add nothing to its counters'
        want.update({'r_ns': r['ns'], 'r_pn': r['pvalues_neg'], 'r_pp': r['pvalues_pos'], 'r_nes': r['nes'], 'r_nb': r['nes_binary'],
                     'r_enriched': r['num_neighborhoods_enriched']})
    if 'score' in entries:
        want['s_ns'] = ns
    return want


# ------------------------------------------------------------------------------------------------ 0. the switch ----

def test_the_switch_sets_the_planning_count_and_nothing_else_does(be, plans):
    full = max(plans)
    assert [plans[k].num_cu for k in pl.SMALL_CUS] == list(pl.SMALL_CUS)
    for value in (None, '', '0', '-1', 'abc', '2x', '1.5', str(full + 1), '99999999999999999999'):
        ctx = context_with(be, value)
        try:
            assert ctx.num_cu == full, value
        finally:                                                        # (nothing was allocated on it)
            be.check(be.lib.safe_ctx_destroy(ctx.handle))
            ctx.handle = None
    assert os.environ.get(VAR) is None or plans[full].num_cu == full
    assert be.Context.default(0) is plans[full]


# --------------------------------------------------------------------------------- 1. weighted counts and score ----

def weighted_input():
    n, m = pl.WEIGHTED['n'], pl.WEIGHTED['m']
    a = tm.membership(n, 5, dense_row=True)                             # slices of very different widths; an empty row
    indptr, indices = wr.csr_of(a)
    rng = np.random.default_rng(6)
    w = np.round(rng.uniform(size=len(indices)) * 16) / 16
    w[::4] = 0.0                                                        # zero weights stay members
    return a, indptr, indices, w, quantitative(n, m, 7)


def test_weighted_counts_and_score(be, plans):
    assert_plan('weighted', plans)
    n, m, n_perm = (pl.WEIGHTED[k] for k in ('n', 'm', 'n_perm'))
    a, indptr, indices, w, b = once('weighted', weighted_input)
    outs = {}
    for k, ctx in plans.items():
        nbr = be.Neighborhoods.from_dense(ctx, a)
        attr = be.Attributes.from_host(ctx, b)
        attr_f = be.Attributes.from_host(ctx, np.asfortranarray(b))
        perms = be.Permutations(ctx, n, attr.row_flags(), n_perm, SEED)
        cell = ((n, m), F64)
        out = tm.Poisoned(ctx, {'ns': cell, 'neg': cell, 'pos': cell, 'score': cell})
        try:
            assert np.array_equal(nbr.csr()[1], indices)
            nbr.set_weights(w)
            be.permtest_counts_weighted(ctx, nbr, attr, perms, out.ptr('ns'), out.ptr('neg'), out.ptr('pos'))
            assert ctx.last_kernel()[0] == 'k_permtest_weighted'
            be.score_weighted(ctx, nbr, attr_f, out.ptr('score'))       # rows contiguous: the tile kernel without a table
            assert ctx.last_kernel()[0] == 'k_permtest_weighted'
            outs[k] = {name: out.read(name) for name in out.shapes}
            outs[k]['tables'] = perms.read()
        finally:
            out.free()
            perms.close()
            attr_f.close()
            attr.close()
            nbr.close()
    tables = outs[pl.SMALL_CUS[0]]['tables']
    x, neg, pos = once('weighted_ref', lambda: wr.counts(indptr, indices, w, b, tables))
    assert (neg != n_perm).any() and (pos != n_perm).any() and (x != 0).any()
    check_plans(outs, {'ns': x, 'neg': neg, 'pos': pos, 'score': x}, 'weighted')


# ------------------------------------------------------------------------------------------------- 2. gather ----

@pytest.mark.parametrize('score', sorted(pl.GATHER))
def test_gather_counts_randomization_and_score(be, plans, monkeypatch, score):
    assert_plan('gather_' + score, plans)
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'gather')
    g = pl.GATHER[score]
    a = tm.membership(g['n'], 5, dense_row=True)
    b = once(('gather_b', score), lambda: quantitative(g['n'], g['m'], 8))
    entries = ('counts', 'randomization', 'score')
    kernel = 'k_permtest_gather<8,true>' if score == 'z-score' else 'k_permtest_gather<16,false>'
    outs = {k: run_enrichment(be, ctx, a, b, score, g['n_perm'], entries, kernel) for k, ctx in plans.items()}
    want = once(('gather_ref', score), lambda: enrichment_reference(a, b, score, g['n_perm'], entries))
    assert np.isnan(want['s_ns']).any() == (score == 'z-score')
    check_plans(outs, want, 'gather ' + score)


# -------------------------------------------------------------------------------------------- 3. maxT extremes ----

def maxt_input():
    n, m = pl.MAXT['n'], pl.MAXT['m']
    a = tm.membership(n, 9)                                             # row 1 is empty: scale = 0 in the first chunk
    a[37] = 0                                                           # and one in the third chunk, which group 0 or 2 walks second
    b = quantitative(n, m, 10)
    b[(~np.isnan(b)).any(axis=1), 17] = 2.5                             # a constant column in the second tile (NaN cells count as 0)
    return a, b


@pytest.mark.parametrize('weighted', [False, True], ids=['flat', 'weighted'])
def test_maxt_extremes_and_counts(be, plans, weighted):
    assert_plan('maxt', plans)
    n, m, n_perm = (pl.MAXT[k] for k in ('n', 'm', 'n_perm'))
    a, b = once('maxt', maxt_input)
    w = tm.custom_weights(a, 3) if weighted else None
    outs, refs = {}, {}
    for k, ctx in plans.items():
        nbr = be.Neighborhoods.from_dense(ctx, a)
        attr = be.Attributes.from_host(ctx, b)
        perms = be.Permutations(ctx, n, attr.row_flags(), n_perm, SEED)
        try:
            if weighted:
                nbr.set_weights(w)
            got = tm.run_extremes(be, ctx, nbr, attr, perms)
            if not refs:
                z, live, tmax, tmin, _ = tm.reference(a, b, w, attr, perms.read().astype(np.int64))
                refs.update({'z': z, 'live': live.astype(U8), 'tmax': tmax, 'tmin': tmin})
                for scope, code in (('neighborhoods', mx.COLUMN), ('all', mx.MATRIX)):
                    for name, arr in zip(('neg', 'pos', 'least_neg', 'least_pos'), mx.counts(z, live, tmax, tmin, code)):
                        refs['%s_%s' % (scope, name)] = arr
            for scope in ('neighborhoods', 'all'):
                for name, arr in zip(('neg', 'pos', 'least_neg', 'least_pos'), tm.run_counts(be, ctx, got, scope)):
                    got['%s_%s' % (scope, name)] = arr
            got['tables'] = perms.read()
            outs[k] = got
        finally:
            perms.close()
            attr.close()
            nbr.close()
    live_rows = refs['live'][:, 0] != 0
    assert not refs['live'][[1, 37]].any() and not refs['live'][:, 17].any()
    assert all(live_rows[c:c + 16].any() for c in range(0, n, 16)), 'a chunk without a live row'
    assert np.isneginf(refs['tmax'][:, 17]).all() and np.isfinite(refs['tmax'][:, :17]).all()
    check_plans(outs, refs, 'maxT ' + ('weighted' if weighted else 'flat'))


# ------------------------------------------------------------------------------------------------ 4. scatter ----

def scatter_input(n, m, seed, hub=False):
    """0/1 columns whose neighbours in the queue order (descending support) differ as much as they can: all ones, half full,
    sparse, one-hot and empty columns, so that a workgroup goes from a column that touches every counter to one that touches
    almost none; rows without a value."""
    rng = np.random.default_rng(seed)
    if hub:                                                             # test_gpu_routes.py 'bin_hub': one neighborhood holds every node
        a = (rng.uniform(size=(n, n)) < 0.004).astype(np.int64)
        a[5, :] = 1
    else:
        a = orc.neighborhoods_euclidean(rng.uniform(size=(n, 2)), 0.1)
    density = np.resize([1.0, 0.0, 0.5, -1.0, 0.05], m)                 # -1: one-hot
    b = np.zeros((n, m))
    for j, d in enumerate(density):
        if d < 0:
            b[rng.integers(0, n), j] = 1.0
        else:
            b[:, j] = rng.uniform(size=n) < d
    b[rng.choice(n, n // 30, replace=False)] = np.nan
    return a, b


@pytest.mark.parametrize('case', ['scatter', 'scatter_hub'])
def test_scatter_counts_and_randomization(be, plans, monkeypatch, case):
    assert_plan(case, plans)
    monkeypatch.setenv('SAFE_HIP_FORCE_PATH', 'scatter')
    g = pl.SCATTER_HUB if case == 'scatter_hub' else pl.SCATTER
    a, b = once(case, lambda: scatter_input(g['n'], g['m'], 12, hub=case == 'scatter_hub'))
    entries = ('counts', 'randomization')
    outs = {k: run_enrichment(be, ctx, a, b, 'sum', g['n_perm'], entries, 'k_permtest_scatter') for k, ctx in plans.items()}
    want = once(case + '_ref', lambda: enrichment_reference(a, b, 'sum', g['n_perm'], entries))
    support = np.nansum(b, axis=0)
    assert support.max() >= 0.9 * g['n'] and (support == 1).any() and (support == 0).any()
    assert (want['c_pos'] != g['n_perm']).any() and (want['c_neg'] != g['n_perm']).any()
    check_plans(outs, want, case)


# ------------------------------------------------------------------------------------------------ 5. LDS f64 ----

@pytest.mark.parametrize('score', sorted(pl.LDS))
def test_lds_f64_counts_and_randomization(be, plans, score):
    assert_plan('lds_' + score, plans)
    g = pl.LDS[score]
    a = tm.membership(g['n'], 13)
    b = once(('lds_b', score), lambda: quantitative(g['n'], g['m'], 14))
    entries = ('counts', 'randomization')
    outs = {k: run_enrichment(be, ctx, a, b, score, g['n_perm'], entries, 'k_permtest_lds') for k, ctx in plans.items()}
    want = once(('lds_ref', score), lambda: enrichment_reference(a, b, score, g['n_perm'], entries))
    check_plans(outs, want, 'lds ' + score)


# ----------------------------------------------------------------------------------------- 6. radius selection ----

def percentile_ranks(count):
    """The two order statistics np.percentile interpolates between, for every q of radius_ref.QS."""
    pos = [q / 100.0 * (count - 1) for q in rr.QS]
    return sorted({int(np.floor(p)) for p in pos} | {int(np.ceil(p)) for p in pos})


def test_radius_selection_on_a_layout(plans):
    assert_plan('select_xy', plans)
    n = pl.SELECT['n']
    xy = rr.xy_input('uniform', n)
    sv = rr.sorted_pdist(xy)
    ranks = np.concatenate([rr.ranks_for(sv, extra=8, seed=1), percentile_ranks(sv.shape[0])]).astype(np.int64)
    sc = nrf.sorted_candidates(nrf.euclid(xy), False)
    outs = {}
    for k, ctx in plans.items():
        got, count = ctx.pair_distance_select(xy, ranks)
        assert count == sv.shape[0] == ctx.pair_distance_select(xy, [])[1]
        outs[k] = {'percentile': got}
        outs[k].update({'nearest_%d' % kk: ctx.row_distance_select(xy, kk) for kk in nrf.ks_for(n)})
    want = {'percentile': sv[ranks]}
    want.update({'nearest_%d' % kk: nrf.radii_from_sorted(sc, kk) for kk in nrf.ks_for(n)})
    check_plans(outs, want, 'selection from coordinates')


def test_radius_selection_on_a_graph_distance_source(amd, plans):
    assert_plan('select_dist', plans)
    n = pl.SELECT['n']
    g = nrf.component_graph(n)
    d = once('select_graph', lambda: sr.scipy_reference(g, np.inf)[1])
    sv = rr.finite_upper(d)
    ranks = np.concatenate([rr.ranks_for(sv, extra=8, seed=2), percentile_ranks(sv.shape[0])]).astype(np.int64)
    sc = nrf.sorted_candidates(d, True)
    outs = {}
    for k, ctx in plans.items():
        nbr = amd.Neighborhoods.shortpath(ctx, g.n, g.eu, g.ev, g.ew, np.inf, keep_distances=True)
        try:
            got, count = nbr.distance_select(ranks)
            assert count == sv.shape[0]
            outs[k] = {'distances': nbr.distances(), 'percentile': got}
            outs[k].update({'nearest_%d' % kk: nbr.row_distance_select(kk) for kk in nrf.ks_for(n)})
        finally:
            nbr.close()
    want = {'distances': d, 'percentile': sv[ranks]}
    want.update({'nearest_%d' % kk: nrf.radii_from_sorted(sc, kk) for kk in nrf.ks_for(n)})
    check_plans(outs, want, 'selection from a kept matrix')


# ------------------------------------------------------------------------------------ 7. plans already pinned ----

@pytest.mark.parametrize('cutoff', [1.0, np.inf], ids=['bounded', 'unbounded'])
@pytest.mark.parametrize('weights', ['dyadic', 'real'])
def test_shortest_paths_with_a_dozen_sources_per_worker(amd, plans, weights, cutoff):
    """shortpath_ref.rung_graph(40, 1), n = 101, on 8 workers: each serves 12 or 13 sources on one scratch."""
    assert_plan('shortpath', plans)
    g = sr.rung_graph(pl.SHORTPATH['workers'], 1, weights)
    assert g.n == pl.SHORTPATH['n']
    want_a, want_d = once(('rung', weights, cutoff),
                          lambda: sr.oracle_reference(g, cutoff) if np.isfinite(cutoff) else sr.scipy_reference(g, cutoff))
    first = None
    for k, ctx in plans.items():
        got = ts._run(amd, ctx, g, cutoff)
        ts._check(got, want_a, want_d, '%d CUs' % k)
        first = first or got
        ts._identical(first, got, '%d CUs' % k)


@pytest.mark.parametrize('kind', ['uniform', 'lattice'])
def test_dense_euclidean_sweep_in_whole_batches_on_one_cu(plans, kind):
    """prep_ref.dense_sizes(1): both sides of n = 29, the first size at which one CU's four workgroups take whole batches."""
    ctx = plans[1]
    nb, sizes = pr.dense_sizes(ctx.num_cu)
    assert nb == 29 and any(pr.dense_geometry(n, ctx.num_cu)[2] for n in sizes.values())
    assert not any(pr.dense_geometry(n, max(plans))[2] for n in sizes.values())
    for n in sorted(set(sizes.values())):
        xy = pr.xy_input(kind, n)
        nr = pr.XY_RADIUS[kind]
        want_d = orc.euclidean_distances(xy)
        want_m = (want_d < nr).astype(np.int64)
        tp.run_dense(ctx, xy, nr, want_m, None)
        tp.run_dense(ctx, xy, nr, None, want_d)
        tp.run_dense(ctx, xy, nr, want_m, want_d)


# ------------------------------------------------------------------------------------------------ 8. every route ----

@pytest.fixture(scope='module')
def route_data(be, plans):
    full = max(plans)
    data = {k: {kind: tr.make_data(be, plans[k], kind) for kind in tr.DATA} for k in (1, full)}
    yield data
    for per_ctx in data.values():
        for nbr, attr, _, _ in per_ctx.values():
            attr.close()
            nbr.close()


@pytest.mark.parametrize('case', tr.CASES, ids=[tr._case_id(*c) for c in tr.CASES])
def test_routes_and_outputs_do_not_depend_on_the_plan(be, plans, route_data, monkeypatch, case):
    """Every case of test_gpu_routes.py on one planning CU and on the whole chip: the same kernel family (routes do not read the
    CU count) and the same SHA-256 over all outputs -- the matrix-core and bit-sliced task queues at a small plan."""
    runs = {k: tr.run_case(be, plans[k], route_data[k], *case, monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
            for k in route_data}
    (name_1, plan_1, digest_1), (name_f, plan_f, digest_f) = runs[1], runs[max(plans)]
    assert name_1 == name_f == tr.EXPECTED[tr._case_id(*case)]
    assert plan_1 == plan_f
    assert digest_1 == digest_f, 'the outputs of %s depend on the planning CU count' % name_1
