"""The two-tailed hypergeometric reference (tests/hyp_tails_ref.py) and the host side of hypergeom_tails where no GPU exists:
the exact lower tail against its mirror identity and against SciPy's cdf on the cells the GPU test uses, the setting in
validate_config and through a pickle, and the three new symbols in the header, the binding and the library."""
import ctypes
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest

import hyp_cases as hc
import hyp_exact as hx
import hyp_tails_ref as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lower_tail_is_the_upper_tail_of_the_mirrored_draw():
    """P[H <= x | pop, K, n] = P[H' >= n - x | pop, pop - K, n] on every designed triple, and the support rules of scipy's cdf."""
    count = 0
    for c in hc.all_cases():
        for K, n, x in c.triples():
            assert ht.exact_lower_tail(c.pop, K, n, x) == hx.exact_tail(c.pop, c.pop - K, n, n - x), (c.name, K, n, x)
            count += 1
    assert count > 30000
    assert ht.exact_lower_tail(10, 7, 6, 2) == 0 and ht.exact_lower_tail(10, 7, 6, 3) > 0      # support 3 .. 6
    assert ht.exact_lower_tail(10, 7, 6, 5) < 1 and ht.exact_lower_tail(10, 7, 6, 6) == 1 and ht.exact_lower_tail(10, 7, 6, 9) == 1


def test_lower_tail_against_scipy_cdf_on_the_mirrored_triples():
    from scipy.stats import hypergeom
    worst, cells = 0.0, 0
    for c in hc.all_cases():
        keys = [(c.pop - K, n, n - x) for K, n, x in c.triples()]
        K, n, x = (np.array(v, dtype=np.int64) for v in zip(*keys))
        got = hypergeom.cdf(x, c.pop, K, n)
        for t, g in zip(keys, got):
            e = ht.exact_lower_tail(c.pop, *t)
            assert 0.0 <= g <= 1.0
            cells += 1
            if e >= Fraction(1, 10 ** 290):
                rel = float(abs(Fraction(float(g)) - e) / e)
                worst = max(worst, rel)
                assert rel <= 1e-12, (c.name, t, g, float(e))
    print('scipy.stats.hypergeom.cdf against the exact lower tail: worst relative difference %.3g over %d triples' % (worst, cells))


def test_numpy_restatement_and_exact_decisions_agree_on_plain_cells():
    p_pos = np.array([[1.0, 0.5, 1e-3, 0.0, 0.04, np.nan]])
    p_neg = np.array([[1e-4, 0.6, 1.0, 1.0, 0.9, 0.5]])
    for sign, want in (('highest', [0, 0, 1, 1, 1, 0]), ('lowest', [1, 0, 0, 0, 0, 0]), ('both', [1, 0, 1, 1, 1, 0])):
        v, nb, counts = ht.outputs(p_pos, p_neg, sign, 0.05)
        assert nb.tolist() == [[float(w) for w in want]], sign
        assert np.array_equal(counts, nb.sum(axis=0))
    assert ht.nes(np.array([0.0]), np.array([1.0]), 'both')[0] == np.inf and ht.nes(np.array([1.0]), np.array([0.0]), 'both')[0] == -np.inf
    thr = Fraction(1, 20)
    assert ht.exact_decision(thr, Fraction(1), 'highest', thr) == (False, False)                # p == threshold: kept, not enriched
    assert ht.exact_decision(thr * (1 - Fraction(1, 10 ** 7)), Fraction(1), 'highest', thr) == (False, True)
    assert ht.exact_decision(Fraction(1, 100), Fraction(1), 'highest', thr) == (True, False)
    assert ht.exact_decision(Fraction(1), Fraction(1, 100), 'lowest', thr) == (True, False)
    assert ht.exact_decision(Fraction(1), Fraction(1, 100), 'highest', thr) == (False, False)
    assert ht.exact_decision(Fraction(1, 2), Fraction(1, 50), 'both', thr) == (True, False)     # ratio 1 / 25 < 1 / 20
    assert ht.exact_decision(Fraction(1, 50), Fraction(1, 2), 'both', thr) == (True, False)     # ratio 25 > 20
    assert ht.exact_decision(Fraction(1, 2), Fraction(1, 30), 'both', thr) == (False, False)    # ratio 1 / 15
    assert ht.exact_decision(Fraction(1, 40), Fraction(1, 2), 'both', thr)[1]                   # ratio 20: on the bound
    assert ht.exact_decision(Fraction(0), Fraction(1), 'both', thr) == (True, False)


def test_validate_config_and_pickle_keep_the_setting():
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    assert sf.hypergeom_tails == 'upper'
    sf.hypergeom_tails = 'attribute_sign'
    sf.validate_config()
    assert sf.hypergeom_tails == 'attribute_sign'
    back = pickle.loads(pickle.dumps(sf))
    assert back.hypergeom_tails == 'attribute_sign'
    back.validate_config()
    for bad in ('lower', 'both', None, 1):
        sf.hypergeom_tails = bad
        with pytest.raises(ValueError, match='hypergeom_tails'):
            sf.validate_config()
        assert sf.hypergeom_tails == 'upper'                    # restored, like the other checks
    # an object pickled before the setting existed
    state = sf.__getstate__()
    del state['hypergeom_tails']
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert old.hypergeom_tails == 'upper'
    # the sharded paths never read it
    for name in ('sharding.py', 'run_batch.py'):
        assert 'hypergeom_tails' not in open(os.path.join(ROOT, 'safepy_amd', name)).read()


def test_header_binding_and_library_agree_on_the_new_symbols():
    from safepy_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert '#define SAFE_HIP_ABI_VERSION 9' in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want_args = {'safe_hypergeom_tails': 14, 'safe_hypergeom_outputs': 10, 'safe_fdr_adjust_rows': 4}
    for name, n_args in want_args.items():
        m = re.search(r'\bint %s\s*\(([^;]*)\);' % name, code)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, name
        assert hasattr(raw, name), name
    tails = _lib.PROTOTYPES['safe_hypergeom_tails'][1]
    assert tails[3] is ctypes.c_int and tails[4] is ctypes.c_double and tails[5] is ctypes.c_int
    assert tails[6] is ctypes.c_int64 and tails[7] is ctypes.c_int64
    # the header's list of entry points that return only once the stream has drained names all three
    conventions = header[:header.index('#ifndef SAFE_HIP_H')]
    for name in want_args:
        assert name in conventions, name
