"""k_spring_step (layout.hip) through Context.layout_spring against tests/layout_ref.py's fr_ref, the NumPy restatement of
networkx 3.4.2's two Fruchterman-Reingold iterations that tests/test_layout_ref_cpu.py holds to the real library: the
bits of every coordinate and the number of iterations run, on

  - sizes on both sides of every tile (16 rows) and chunk (128 columns) edge in both forms, 1 ... 2049 nodes
  - dense graphs, whose (tile, chunk) neighbour lists exceed one and two rounds of the 256-thread scatter
  - start positions that reach both clamps (coincident and near pairs, d == 0.01 and one ulp either side, zero net force)
  - zero, negative, self-loop, absent and not-f32-representable weights
  - k and iteration counts other than 0.2 and 100
  - thresholds that stop the run after an odd and after an even iteration
  - the refusals, inputs left alone, and two calls giving the same bits.

No tolerance anywhere: bit equality is the kernel's contract.  The references are computed once per process
(layout_ref.reference) and are read-only."""
import numpy as np
import pytest

import layout_ref as L

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


@pytest.fixture(scope='module')
def ctx():
    import safepy_amd
    from safepy_amd import backend as be
    assert safepy_amd.device_count() >= 1
    return be.Context.default(0)


def run(ctx, case):
    return ctx.layout_spring(case['row_ptr'], case['col'], case['weight'], case['pos0'], case['k'], case['iterations'],
                             case['threshold'], case['dtype'])


def check(ctx, case):
    """The device's positions and iteration count equal fr_ref's; returns (fr_ref's stats, iterations run)."""
    want, want_ran, stats = L.reference(case)
    got, ran = run(ctx, case)
    differ = int((got != want).sum()) if got.shape == want.shape else -1
    print('%s: n=%d iterations=%d ran=%d (reference %d) coordinates that differ: %d' %
          (case['name'], case['n'], case['iterations'], ran, want_ran, differ))
    assert got.dtype == want.dtype == case['dtype'] and got.shape == want.shape == (case['n'], 2)
    assert np.isfinite(want).all()
    assert np.array_equal(got, want), '%s: %d of %d coordinates differ' % (case['name'], differ, want.size)
    assert ran == want_ran, '%s: ran %d iterations, the reference %d' % (case['name'], ran, want_ran)
    assert stats['stop_margin'] > 1e-6          # no stop decision hung on the order of the sum of squares
    return stats, ran


def family(prefixes):
    cases = [c for c in L.all_cases() if c['name'].startswith(prefixes)]
    return pytest.mark.parametrize('case', cases, ids=[c['name'] for c in cases])


SIZE_CASES = [c for c in L.all_cases() if c['name'].startswith(('f64-n', 'f32-n'))]


@family(('f64-n', 'f32-n'))
def test_size_sweep(ctx, case):
    if case['dtype'] == F32:
        assert case['n'] * case['iterations'] <= L.F32_BUDGET
    check(ctx, case)


def test_size_sweep_lists():
    got = {(c['dtype'], c['n'], c['iterations']) for c in SIZE_CASES}
    assert {(F64, n, 100) for n in L.SIZES_F64} <= got
    assert {(F32, n) for n in L.SIZES_F32} | {(F32, 16), (F32, 129), (F32, 256)} == {(d, n) for d, n, _ in got if d == F32}
    assert {(F32, n, 100) for n in (16, 129, 256)} | {(F64, 640, 10), (F64, 1025, 10)} <= got
    for n in L.SIZES_F64[3:] + L.SIZES_F32:                      # every listed size sits on or next to a tile or chunk edge
        assert n % 16 in (0, 1, 15) or n % 128 in (0, 1, 127) or n in (499, 500), n
    assert max(L.SIZES_F64) < 500 <= min(L.SIZES_F32)
    # N = 1: nothing but its own term, a short force, the node stays where it is
    want, ran, stats = L.reference(L.case_named('f64-n1'))
    assert np.array_equal(want, L.case_named('f64-n1')['pos0']) and stats['first_len_rows'] == {0}


@family('dense-')
def test_dense_graphs(ctx, case):
    """More than 256 and more than 512 entries in a (16-row, 128-column) block: the scatter's second and third rounds,
    in chunk 0's loop and in the loop behind the prefetched first entry."""
    occ = L.block_occupancy(case['row_ptr'], case['col'])
    assert occ.sum() == case['col'].size
    assert (occ > 256).any() and (occ > 512).any(), occ.max()
    check(ctx, case)


def test_dense_cases_reach_both_scatter_loops():
    """Chunk 0's list is scattered by one loop, every later chunk's by the loop behind the prefetched first entry: in each
    form some case has more than 512 entries in a block of either kind; one case has a block that ends inside the second
    round and one a block of exactly 256 entries."""
    for dtype in (F64, F32):
        occ = [L.block_occupancy(c['row_ptr'], c['col']) for c in L.dense_cases() if c['dtype'] == dtype]
        assert any((o[:, 0] > 512).any() for o in occ) and any((o[:, 1:] > 512).any() for o in occ)
    occ = [L.block_occupancy(c['row_ptr'], c['col']) for c in L.dense_cases()]
    assert any(((o > 256) & (o <= 512)).any() for o in occ) and any((o == 256).any() for o in occ)


@family('clamp-')
def test_clamps(ctx, case):
    stats, ran = check(ctx, case)
    expect = case['expect']
    T = case['dtype'].type
    pos = case['pos0'].astype(case['dtype'])
    for (i, j), d in expect.get('distances', {}).items():          # d of the designed pairs is what the case says
        dx, dy = pos[i, 0] - pos[j, 0], pos[i, 1] - pos[j, 1]
        assert np.sqrt(dx * dx + dy * dy) == T(d)
    if 'distances' in expect:
        at, below, above = (expect['distances'][p] for p in ((0, 1), (2, 3), (4, 5)))
        assert T(at) == T(0.01) and T(below) == np.nextafter(T(0.01), T(0)) and T(above) == np.nextafter(T(0.01), T(1))
    assert expect.get('clamped', set()) <= stats['first_clamped_pairs']
    assert not (expect.get('not_clamped', set()) & stats['first_clamped_pairs'])
    if expect.get('clamped'):
        assert stats['d_clamped'] >= len(expect['clamped'])
    if expect.get('zero'):
        assert stats['d_zero'] >= 2                                 # a coincident pair: dx == dy == 0, both directions
    assert expect.get('short_rows', set()) <= stats['first_len_rows']
    if expect.get('short_rows'):
        assert stats['len_clamped'] >= len(expect['short_rows'])
    if 'ran' in expect:
        assert ran == expect['ran']
    assert case['n'] <= 40 and case['iterations'] == 100


def test_clamp_cases_reach_every_branch():
    names = {c['name'] for c in L.clamp_cases()}
    assert names == {'clamp-%s-%s' % (a, b) for a in ('coincident3', 'near', 'ulp', 'zero2', 'cross') for b in ('f64', 'f32')}
    for tag in ('f64', 'f32'):
        stats = L.reference(L.case_named('clamp-coincident3-' + tag))[2]
        assert stats['d_zero'] >= 2 * 100                          # nodes 0 and 1 stay coincident through all 100 iterations
        stats = L.reference(L.case_named('clamp-cross-' + tag))[2]
        assert stats['first_len_rows'] == {0} and stats['d_clamped'] == 0


@family('weights-')
def test_weights(ctx, case):
    rp, col, w, A = case['row_ptr'], case['col'], case['weight'], case['A']
    rows = np.repeat(np.arange(case['n']), np.diff(rp))
    name = case['name']
    if 'zero' in name:
        assert w is not None and int((w == 0).sum()) == case['stored_zeros'] > 0 and (w != 0).any()
    elif 'negative' in name:
        assert (w < 0).sum() > 10 and (w > 0).sum() > 10
    elif 'selfloop' in name:
        assert (rows == col).sum() == 2 and (w[rows == col] != 0).all()
    elif 'none' in name:
        assert w is None and set(np.unique(A)) == {0.0, 1.0}
    elif 'rounding' in name:
        assert case['dtype'] == F32 and (w != 1.0).all() and (w.astype(np.float32) == 1.0).all()
    else:
        raise AssertionError(name)
    if w is not None and 'rounding' not in name:                   # uniform(0.5, 2) draws: rounding to f32 changes them
        assert (w.astype(np.float32).astype(np.float64) != w)[w != 0].mean() > 0.9
    check(ctx, case)


def test_weight_cases_cover_both_forms():
    names = {c['name'] for c in L.weight_cases()}
    assert {'weights-%s-%s' % (a, b) for a in ('zero', 'negative', 'selfloop', 'none') for b in ('f64-n60', 'f32-n520')} | \
        {'weights-f32-rounding-f32-n520'} == names


@family(('k0', 'k1', 'it'))
def test_k_and_iterations(ctx, case):
    check(ctx, case)


def test_k_and_iteration_lists():
    cases = L.k_iteration_cases()
    for dtype, n in ((F64, 129), (F32, 513)):
        mine = [c for c in cases if c['dtype'] == dtype]
        assert {c['n'] for c in mine} == {n}
        assert {c['k'] for c in mine} == {0.05, 0.2, 1.0 / 3.0, 1.0}
        want = {1, 2, 3, 50, 101} if dtype == F64 else {1, 2, 3, 50, L.F32_BUDGET // 513}
        assert want <= {c['iterations'] for c in mine}
    assert np.float32(1.0 / 3.0 * (1.0 / 3.0)) != np.float32(1.0 / 3.0) * np.float32(1.0 / 3.0)   # kk = f32(k*k), not f32(k)^2
    assert np.float32(0.2 * 0.2) != np.float32(0.2) * np.float32(0.2)


@family('stop')
def test_early_stop(ctx, case):
    """The threshold lies halfway between two consecutive values of norm(delta) / n = t_it / sqrt(n); the run stops after
    an odd (11) or an even (18) number of iterations, so the half of the position double buffer that is returned is the
    first in one case and the second in the other."""
    stats, ran = check(ctx, case)
    assert ran == case['stop'] and 1 < ran < case['iterations']
    assert stats['len_clamped'] <= 1 and stats['stop_margin'] > 0.02


def test_early_stop_parities():
    cases = L.early_stop_cases()
    assert {(c['dtype'], c['n'], c['stop'] % 2) for c in cases} == {(F64, 144, 0), (F64, 144, 1), (F32, 640, 0), (F32, 640, 1)}


def test_refusals_leave_the_context_usable(ctx):
    from safepy_amd import SafeHipError
    none = np.zeros(0, np.int32)
    pos3 = np.random.RandomState(1).rand(3, 2)
    bad = (
        ("exceed the kernel's limit of 65536", np.zeros(65538, np.int32), none, None, np.zeros((65537, 2)), np.float32),
        ('row_ptr decreases at row 1', np.array([0, 2, 1, 3], np.int32), np.array([1, 2, 0], np.int32), None, pos3, np.float64),
        ('strictly increasing', np.array([0, 2, 2, 2], np.int32), np.array([1, 1], np.int32), None, pos3, np.float64),
        ('strictly increasing', np.array([0, 2, 2, 2], np.int32), np.array([2, 1], np.int32), None, pos3, np.float32),
        ('columns must be in', np.array([0, 0, 1, 1], np.int32), np.array([3], np.int32), np.ones(1), pos3, np.float64),
        ('columns must be in', np.array([0, 0, 1, 1], np.int32), np.array([-1], np.int32), np.ones(1), pos3, np.float32),
        ('dtype must be F32 or F64', np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32), None, pos3, np.float16),
        ('dtype must be F32 or F64', np.array([0, 1, 2, 2], np.int32), np.array([1, 0], np.int32), None, pos3, np.int32),
    )
    for message, rp, col, w, pos0, dtype in bad:
        with pytest.raises(SafeHipError) as err:
            ctx.layout_spring(rp, col, w, pos0, 0.2, 5, 1e-4, dtype)
        assert message in str(err.value), (message, str(err.value))
    check(ctx, L.case_named('f64-n17'))


@pytest.mark.parametrize('name', ['f64-n33', 'weights-selfloop-f32-n520', 'dense-f64-n130-complete'])
def test_inputs_left_alone_and_calls_repeat(ctx, name):
    case = L.case_named(name)
    arrays = {key: case[key].copy() for key in ('row_ptr', 'col', 'weight', 'pos0') if case[key] is not None}
    first, ran1 = run(ctx, case)
    for key, before in arrays.items():
        assert np.array_equal(case[key], before) and case[key].dtype == before.dtype, key
    second, ran2 = run(ctx, case)
    assert ran1 == ran2 and first.tobytes() == second.tobytes()
    want, want_ran, _ = L.reference(case)
    assert ran1 == want_ran and np.array_equal(first, want)
