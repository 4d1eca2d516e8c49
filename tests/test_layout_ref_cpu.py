"""tests/layout_ref.py (the NumPy restatement of networkx's two Fruchterman-Reingold iterations that the GPU sweep of
layout.hip compares with) against the real functions of networkx 3.4.2: the bits of the positions and the number of
iterations run, on the sweep's own cases.  networkx.drawing.layout._fruchterman_reingold (dense, f64) and
_sparse_fruchterman_reingold (f32) are called directly with pos= given, so no rescale_layout follows (safe_io._rescale_layout
is tested with the full path).  Every f64 case runs at its full iterations; networkx's f32 form costs ~190 us per row per
iteration, so an f32 case runs at no more than 15 000 rows x iterations here (a case with a designed stop keeps its
iterations: its threshold belongs to them).  No GPU needed."""
import numpy as np
import pytest

import layout_ref as L

nx = pytest.importorskip('networkx')
if nx.__version__ != '3.4.2':
    pytest.skip('the private layout functions are pinned to networkx 3.4.2, this is %s' % nx.__version__,
                allow_module_level=True)

F32_ROWS_X_ITERATIONS = 15000

F32_NAMES = ('f32-n500', 'f32-n512', 'f32-n640', 'f32-n1025', 'f32-n2049', 'f32-n16', 'f32-n129', 'f32-n256',
             'dense-f32-n513-p0.5', 'dense-f32-n528-complete',
             'clamp-coincident3-f32', 'clamp-near-f32', 'clamp-ulp-f32', 'clamp-zero2-f32', 'clamp-cross-f32',
             'weights-zero-f32-n520', 'weights-negative-f32-n520', 'weights-selfloop-f32-n520',
             'weights-f32-rounding-f32-n520', 'k0.05-f32-n513', 'k0.333-f32-n513', 'it1-f32-n513',
             'it2-f32-n513', 'it3-f32-n513', 'stop11-f32-n640', 'stop18-f32-n640')
# left out for time: the f64 form beyond 500 rows (the raw entry point's; its arithmetic is that of the smaller cases)
# and the two neighbours of 384
F64_LEFT_OUT = ('f64-n640', 'f64-n1025', 'f64-n383', 'f64-n385')


def cpu_cases():
    out = []
    for case in L.all_cases():
        if case['dtype'] == np.dtype(np.float64):
            if case['name'] not in F64_LEFT_OUT:
                out.append(case)
        elif case['name'] in F32_NAMES:
            cap = max(1, F32_ROWS_X_ITERATIONS // case['n'])
            if 'stop' in case:
                assert case['n'] * case['stop'] <= F32_ROWS_X_ITERATIONS          # what it runs before it stops
            elif case['iterations'] > cap:
                case = dict(case, iterations=cap)
            out.append(case)
    return out


CASES = cpu_cases()


def count_norm_calls(fn):
    """fn() and the number of np.linalg.norm calls it made."""
    real = np.linalg.norm
    calls = [0]

    def norm(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    np.linalg.norm = norm
    try:
        out = fn()
    finally:
        np.linalg.norm = real
    return out, calls[0]


def run_networkx(case):
    """(positions, np.linalg.norm calls) of the form of networkx that case['dtype'] selects."""
    from networkx.drawing import layout
    import scipy.sparse as sps
    k, it, thr = case['k'], case['iterations'], case['threshold']
    if case['dtype'] == np.dtype(np.float64):
        A = case['A'].copy()
        return count_norm_calls(lambda: layout._fruchterman_reingold(A, k, case['pos0'].copy(), None, it, thr, 2, None))
    A = sps.csr_array(case['A'].astype(np.float32))               # as to_scipy_sparse_array(G, dtype='f') hands it over
    return count_norm_calls(lambda: layout._sparse_fruchterman_reingold(A, k, case['pos0'].copy(), None, it, thr, 2, None))


@pytest.fixture(scope='module')
def norm_calls_per_iteration():
    """np.linalg.norm calls per iteration of each form, taken on a run that cannot stop early (a negative threshold):
    the dense form takes two row norms and the stop test's, the sparse form the stop test's alone."""
    out = {}
    for name, iterations in (('f64-n17', 7), ('f32-n16', 5)):
        case = dict(L.case_named(name), iterations=iterations, threshold=-1.0)
        _, calls = run_networkx(case)
        assert calls % iterations == 0, (name, calls)
        out[case['dtype']] = calls // iterations
        _, ran = L.fr_ref(case['A'], case['k'], case['pos0'], iterations, -1.0, case['dtype'])
        assert ran == iterations
    assert out == {np.dtype(np.float64): 3, np.dtype(np.float32): 1}, out
    return out


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_equals_networkx_bit_for_bit(case, norm_calls_per_iteration):
    want, calls = run_networkx(case)
    stats = {}
    got, ran = L.fr_ref(case['A'], case['k'], case['pos0'], case['iterations'], case['threshold'], case['dtype'], stats=stats)
    assert want.dtype == got.dtype == case['dtype'] and got.shape == want.shape == (case['n'], 2)
    assert np.array_equal(got, want), '%s: %d coordinates differ' % (case['name'], int((got != want).sum()))
    per = norm_calls_per_iteration[case['dtype']]
    assert calls % per == 0 and ran == calls // per, (ran, calls, per)
    assert stats['stop_margin'] > 1e-6          # no stop decision hung on the order of a sum
    if 'stop' in case:
        assert ran == case['stop'] and 1 < ran < case['iterations']


def test_case_list_covers_both_forms_and_every_family():
    names = [c['name'] for c in CASES]
    assert set(F32_NAMES) <= set(names)
    assert sum(c['dtype'] == np.dtype(np.float64) for c in CASES) == len([c for c in L.all_cases() if c['dtype'] == np.dtype(np.float64)]) - len(F64_LEFT_OUT)
    for family in ('f64-n', 'f32-n', 'dense-', 'clamp-', 'weights-', 'k0.05', 'it3-', 'stop'):
        assert any(n.startswith(family) for n in names), family
    for c in CASES:
        if c['dtype'] == np.dtype(np.float32) and 'stop' not in c:
            assert c['n'] * c['iterations'] <= max(F32_ROWS_X_ITERATIONS, c['n'])
