"""The LDS-resident f64 kernel (k_permtest_lds) and the scatter kernel (k_permtest_scatter) at the limits where perm_route
(safepy_amd/csrc/enrich.hip) hands a permutation test to another family, one case per limit so that a failure names it:

  A  k_permtest_lds with one workgroup owning a CU's whole LDS: N = 4549 fits (163 824 of 163 840 bytes), 4550 does not
  B  k_permtest_lds on small shapes: stride16 on both sides of 8, one slice with fifteen idle waves, 16 / 17 slices
  C  k_permtest_scatter at its LDS limit: N = 16 382 fits (163 836 bytes), 16 383 goes to the bit-sliced form
  D  k_permtest_scatter at its epoch: a neighborhood of 4095 members whose count reaches 4095 in every permutation; 4096 is refused
  E  the scatter kernel's prefetch queue over P: 1, 2 and both sides of every chunk of 16 up to 49
  F  both packed 16-bit counters driven to 65 535 by the kernels themselves; P = 65 536 leaves both routes
  G  caller-supplied tables: identity rows (every counter equals P) and one fixed rotation

Everything is compared with tests/perm_limits_ref.py over the membership read back from the device (Neighborhoods.csr) and the
device's own tables (Permutations.read; the seeded stream itself is pinned to NumPy in tests/test_gpu_seeded_stream.py), every
row, into poisoned buffers with a guard band.  'sum' scores of dyadic or 0/1 values: all outputs EQUAL.  z-scores of normal values:
ns to 1e-9, the counters within the reference's tally of unclear compares -- which tests/test_perm_limits_ref_cpu.py shows to be
zero on every one of these inputs and which is asserted zero here, so in effect equal -- and the fused outputs
from the device's own counters through perm_limits_ref.outputs.  Every case names the kernel it expects after each entry point
and leaves the number of live device blocks where a first run of the same case left it.

The vec_per_row > NT branch of k_permtest_lds needs stride16 / 8 > 1024, N > 8192, beyond what the kernel's LDS admits: no case.
Needs an MI355X."""
import gc
import time

import numpy as np
import pytest

import perm_limits_ref as plr
import test_gpu_maxt as tm
import test_gpu_routes as tr

pytestmark = pytest.mark.gpu

F64 = np.float64
SIGN, THR = 'both', 0.05
LDS, SCATTER, BITS_PRE = 'k_permtest_lds', 'k_permtest_scatter', 'k_permtest_bits_pre'
GATHER_SUM, GATHER_Z = 'k_permtest_gather<16,false>', 'k_permtest_gather<8,true>'
FUSED = ('pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary', 'num_neighborhoods_enriched')


@pytest.fixture(scope='module')
def be():
    import safepy_amd
    from safepy_amd import backend
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return backend


@pytest.fixture(scope='module')
def ctx(be):
    return be.Context.default(0)


@pytest.fixture
def force(monkeypatch):
    """Sets SAFE_HIP_FORCE_PATH (None: unset) and clears every other route switch."""
    def set_to(value):
        for var in tr.SWITCHES.values():
            monkeypatch.delenv(var, raising=False)
        if value is not None:
            monkeypatch.setenv(tr.SWITCHES['F'], value)
    return set_to


def run_device(be, ctx, make_nbr, values, score, perms_of, kernel, read=True):
    """permtest_counts and randomization of one input into poisoned buffers; every handle is closed whatever happens."""
    n, m = values.shape
    cell = ((n, m), F64)
    names = {'c_ns': cell, 'c_neg': cell, 'c_pos': cell,
             'r_ns': cell, 'r_pn': cell, 'r_pp': cell, 'r_nes': cell, 'r_nb': cell, 'r_enriched': ((m,), F64)}
    nbr = attr = perms = out = None
    try:
        nbr = make_nbr()
        attr = be.Attributes.from_host(ctx, values)
        perms = perms_of(attr)
        out = tm.Poisoned(ctx, names)
        ran = []
        be.permtest_counts(ctx, nbr, attr, perms, score, out.ptr('c_ns'), out.ptr('c_neg'), out.ptr('c_pos'))
        ran.append(ctx.last_kernel())
        assert ran[-1][0] == kernel, ('permtest_counts', ran[-1][0])
        be.randomization(ctx, nbr, attr, perms, score, SIGN, THR, [out.ptr(k) for k in list(names)[3:]])
        ran.append(ctx.last_kernel())
        assert ran[-1][0] == kernel, ('randomization', ran[-1][0])
        if not read:
            return None
        got = {name: out.read(name) for name in names}
        got['csr'] = nbr.csr()
        got['tables'] = perms.read().astype(np.int64)
        got['ran'] = ran
        return got
    finally:
        if out is not None:
            out.free()
        for handle in (perms, attr, nbr):
            if handle is not None:
                handle.close()


def run_steady(be, ctx, record_property, what, *args):
    """The case once (its outputs are the ones compared), then once more between two readings of the live device blocks: the
    first run lets the context's scratch and the buffer pool grow to the case's shape, the second must leave nothing behind."""
    t0 = time.perf_counter()
    got = run_device(be, ctx, *args)
    seconds = time.perf_counter() - t0
    gc.collect()                                                        # (handles an earlier test dropped are freed now, not in between)
    before = be.device_live_alloc_count()
    run_device(be, ctx, *args, read=False)
    after = be.device_live_alloc_count()
    for entry, (name, ms, launches) in zip(('permtest_counts', 'randomization'), got['ran']):
        print('%s: %s ran %s (%.3f ms, %d launches); device part of the case %.2f s' % (what, entry, name, ms, launches, seconds))
        record_property('%s %s' % (what, entry), name)
    assert after == before, '%s: %d live device blocks before, %d after' % (what, before, after)
    return got


def seeded(be, ctx, n, n_perm):
    return lambda attr: be.Permutations(ctx, n, attr.row_flags(), n_perm, plr.PERM_SEED)


def euclidean(be, ctx, n, seed, r=None):
    xy = plr.layout(n, seed)
    return lambda: be.Neighborhoods.euclidean(ctx, xy, plr.radius_for(n) if r is None else r)


def equal(got, want, what):
    """np.array_equal with NaN in the same cells."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ': NaN cells'
    bad = np.argwhere((got != want) & ~np.isnan(want))
    assert bad.shape[0] == 0, (what, '%d cells differ, first at' % bad.shape[0], bad[:4].tolist(),
                               [(got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def check_fused(got, ns, neg, pos, n_perm, what):
    want = plr.outputs(ns, neg, pos, n_perm, SIGN, THR)
    for name, key in zip(('r_pn', 'r_pp', 'r_nes', 'r_nb', 'r_enriched'), FUSED):
        equal(got[name], want[key], '%s: %s' % (what, key))


def check_sum(got, values, n_perm, what, reference=None):
    n = values.shape[0]
    assert got['tables'].shape == (n_perm, n)
    if reference is None:
        reference = plr.counts_sum(plr.membership_csr(*got['csr'], n), values, got['tables'])
    ns, neg, pos = reference
    equal(got['c_ns'], ns, what + ': ns')
    equal(got['c_neg'], neg, what + ': counts_neg')
    equal(got['c_pos'], pos, what + ': counts_pos')
    equal(got['r_ns'], ns, what + ': ns of randomization')
    check_fused(got, ns, neg, pos, n_perm, what)
    return ns, neg, pos


def check_z(got, values, n_perm, what):
    n = values.shape[0]
    assert got['tables'].shape == (n_perm, n)
    ns, neg, pos, unclear = plr.counts_z(plr.membership_csr(*got['csr'], n), values, got['tables'])
    print('%s: %d unclear of %d cell-permutations, %d NaN scores' % (what, unclear.sum(), ns.size * n_perm, np.isnan(ns).sum()))
    np.testing.assert_allclose(got['c_ns'], ns, rtol=1e-9, atol=1e-9, equal_nan=True, err_msg=what)
    assert np.all(np.abs(got['c_neg'] - neg) <= unclear) and np.all(np.abs(got['c_pos'] - pos) <= unclear), what
    ok = unclear == 0
    assert np.array_equal(got['c_neg'][ok], neg[ok]) and np.array_equal(got['c_pos'][ok], pos[ok]), what
    assert unclear.sum() == 0, what
    equal(got['r_ns'], got['c_ns'], what + ': ns of randomization')
    check_fused(got, got['c_ns'], got['c_neg'], got['c_pos'], n_perm, what)
    return ns, neg, pos


# ----------------------------------------------------------------------------- A. LDS f64 at the LDS limit ----

LIMIT_CASES = [(n, score, 'lds') for n in (plr.LDS_F64_MAX_N, plr.LDS_F64_MAX_N + 1) for score in ('sum', 'z-score')]
LIMIT_CASES.append((plr.LDS_F64_MAX_N, 'sum', None))                    # the narrow rule: the route a user gets


@pytest.mark.parametrize('n,score,switch', LIMIT_CASES, ids=['%d-%s-%s' % (n, s, 'F=lds' if f else 'default') for n, s, f in LIMIT_CASES])
def test_lds_f64_at_the_lds_limit(be, ctx, force, record_property, n, score, switch):
    fits = plr.lds_f64_bytes(n) <= plr.LDS_BUDGET
    assert fits == (n == 4549)
    kernel = LDS if fits else (GATHER_Z if score == 'z-score' else GATHER_SUM)
    n_perm = 12
    force(switch)
    what = 'lds limit N=%d %s %s' % (n, score, switch)
    if score == 'sum':
        values = plr.dyadic(n, 5, 70)
        got = run_steady(be, ctx, record_property, what, euclidean(be, ctx, n, n), values, score, seeded(be, ctx, n, n_perm), kernel)
        _, neg, pos = check_sum(got, values, n_perm, what)
    else:
        _, m, n_perm, _, layout_seed, value_seed = plr.Z_LIMIT_CASES['lds_%d' % n]
        values = plr.normal(n, m, value_seed)
        got = run_steady(be, ctx, record_property, what, euclidean(be, ctx, n, layout_seed), values, score, seeded(be, ctx, n, n_perm), kernel)
        _, neg, pos = check_z(got, values, n_perm, what)
    members = np.diff(got['csr'][0])
    assert 10 <= members.mean() <= 40 and (neg != n_perm).any() and (pos != n_perm).any()


# ------------------------------------------------------------------------------ B. LDS f64 small shapes ----

SMALL_CASES = [(n, score) for n in plr.SMALL_NS for score in ('sum', 'z-score')] + [(300, 'z-score')]


@pytest.mark.parametrize('n,score', SMALL_CASES, ids=['%d-%s' % c for c in SMALL_CASES])
def test_lds_f64_small_shapes(be, ctx, force, record_property, n, score):
    """(N = 300 with five z-score columns is the input whose tolerance cap the CPU file checks by name.)"""
    if n == 300:
        _, m, n_perm, r, layout_seed, value_seed = plr.Z_LIMIT_CASES['n300']
        assert (n_perm, r) == (plr.SMALL_PERMS, plr.SMALL_RADIUS)
        inputs = [(None, plr.layout(n, layout_seed), plr.normal(n, m, value_seed))]
    else:
        inputs = [plr.small_case(n, score, m) for m in ((1, 3, 4, 5) if score == 'sum' else (1, 2))]
    force('lds')
    for a, xy, values in inputs:
        m = values.shape[1]
        what = 'small N=%d %s m=%d' % (n, score, m)
        make = (lambda: be.Neighborhoods.from_dense(ctx, a)) if a is not None else (lambda: be.Neighborhoods.euclidean(ctx, xy, plr.SMALL_RADIUS))
        got = run_steady(be, ctx, record_property, what, make, values, score, seeded(be, ctx, n, plr.SMALL_PERMS), LDS)
        if a is not None:
            assert np.array_equal(plr.membership_csr(*got['csr'], n).toarray(), a)
        if score == 'sum':
            check_sum(got, values, plr.SMALL_PERMS, what)
        else:
            check_z(got, values, plr.SMALL_PERMS, what)


# ----------------------------------------------------------------------------- C. scatter at the LDS limit ----

@pytest.mark.parametrize('n', [plr.SCATTER_MAX_N, plr.SCATTER_MAX_N + 1])
def test_scatter_at_the_lds_limit(be, ctx, force, record_property, n):
    fits = plr.scatter_bytes(n) <= plr.LDS_BUDGET
    assert fits == (n == 16382)
    n_perm = 17
    values = plr.binary(n, 6, 80, np.geomspace(0.002, 0.3, 6))
    force('scatter')
    what = 'scatter limit N=%d' % n
    got = run_steady(be, ctx, record_property, what, euclidean(be, ctx, n, n), values, 'sum', seeded(be, ctx, n, n_perm),
                     SCATTER if fits else BITS_PRE)
    _, neg, pos = check_sum(got, values, n_perm, what)
    assert (neg != n_perm).any() and (pos != n_perm).any() and np.diff(got['csr'][0]).max() >= 15


# -------------------------------------------------------------------------- D. scatter at the member limit ----

@pytest.mark.parametrize('biggest', [plr.SCATTER_MAX_MEMBERS, plr.SCATTER_MAX_MEMBERS + 1])
def test_scatter_at_the_member_limit(be, ctx, force, record_property, biggest):
    n, n_perm = 4200, 17
    a = plr.hub_membership(n, biggest, 90)
    values = plr.binary(n, 6, 91, [1.0, 0.99, 0.3, 0.01, 0.0, 0.0], nan_rows=False)
    values[1234, 4] = 1.0                                               # one single 1; the last column stays empty
    assert values[:, 0].all() and values[:, 4].sum() == 1 and not values[:, 5].any() and not np.isnan(values).any()
    force(None)
    what = 'scatter members=%d' % biggest
    got = run_steady(be, ctx, record_property, what, lambda: be.Neighborhoods.from_dense(ctx, a), values, 'sum',
                     seeded(be, ctx, n, n_perm), SCATTER if biggest == 4095 else LDS)
    assert np.array_equal(np.diff(got['csr'][0]), a.sum(axis=1))
    ns, neg, pos = check_sum(got, values, n_perm, what)
    # the all-ones column drives the hub's running count to its member count in every permutation, and ties there
    assert ns[0, 0] == biggest and ns[1, 0] == biggest - 1 and neg[0, 0] == pos[0, 0] == n_perm
    assert (neg != n_perm).any() and (pos != n_perm).any()


# --------------------------------------------------------------------------- E. scatter pipeline over P ----

@pytest.mark.parametrize('n_perm', plr.SWEEP_PERMS)
def test_scatter_pipeline_over_p(be, ctx, force, record_property, n_perm):
    n = 300
    values = plr.binary_supports(n, plr.SWEEP_SUPPORTS, plr.SWEEP_SEED)
    force('scatter')
    what = 'scatter P=%d' % n_perm
    got = run_steady(be, ctx, record_property, what, euclidean(be, ctx, n, n), values, 'sum', seeded(be, ctx, n, n_perm), SCATTER)
    _, neg, pos = check_sum(got, values, n_perm, what)
    assert (neg != n_perm).any() and (pos != n_perm).any()


# ----------------------------------------------------------------------- F. saturated packed counters ----

@pytest.mark.parametrize('n_perm', [plr.PACKED_MAX_P, plr.PACKED_MAX_P + 1])
@pytest.mark.parametrize('family', ['scatter', 'lds'])
def test_saturated_packed_counters(be, ctx, force, record_property, family, n_perm):
    a, bits, quant = plr.saturation_inputs()
    values = bits if family == 'scatter' else quant
    n = plr.SATURATION_N
    kernel = GATHER_SUM if n_perm > plr.PACKED_MAX_P else SCATTER if family == 'scatter' else LDS
    force(family)
    what = '%s P=%d' % (family, n_perm)
    got = run_steady(be, ctx, record_property, what, lambda: be.Neighborhoods.from_dense(ctx, a), values, 'sum',
                     seeded(be, ctx, n, n_perm), kernel)
    assert got['tables'].shape == (n_perm, n)
    ns, neg, pos = check_sum(got, values, n_perm, what, reference=plr.counts_sum_batched(a, values, got['tables']))
    full = (neg == n_perm) & (pos == n_perm)
    assert full[:, 1].all() and full.sum() >= n, 'the reference has no cell with both counters at P'
    assert (neg < n_perm).any() and (pos < n_perm).any()


# ------------------------------------------------------------------------------------ G. designed tables ----

@pytest.mark.parametrize('shift', [0, 1], ids=['identity', 'rotation'])
@pytest.mark.parametrize('family', ['scatter', 'lds'])
def test_designed_tables(be, ctx, force, record_property, family, shift):
    """A handle over a caller's table keeps a 16-bit copy for N < 65 535 (safe_perms_create_from_table), so both kernels serve it."""
    n, n_perm = 300, 17
    values = plr.binary(n, 6, 110, [0.5, 0.05, 1.0, 0.0, 0.2, 0.01]) if family == 'scatter' else plr.dyadic(n, 4, 111)
    table = plr.rotation_table(n, n_perm, shift)
    force(family)
    what = '%s table shift=%d' % (family, shift)
    got = run_steady(be, ctx, record_property, what, euclidean(be, ctx, n, n), values, 'sum',
                     lambda attr: be.Permutations.from_table(ctx, table), SCATTER if family == 'scatter' else LDS)
    assert np.array_equal(got['tables'], table)
    _, neg, pos = check_sum(got, values, n_perm, what)
    if shift == 0:
        assert (neg == n_perm).all() and (pos == n_perm).all()
        assert (got['c_neg'] == n_perm).all() and (got['c_pos'] == n_perm).all()
    else:
        assert (neg != n_perm).any() and (pos != n_perm).any()
