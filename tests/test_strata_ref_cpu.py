"""permutation_strata without a GPU: the NumPy restatement of the restricted permutation stream (tests/strata_ref.py) against
the oracle's device stream and against what any restricted permutation must be, the 'neighborhood_size' binning against a
hand-worked example, and the settings, INI keys, pickling and symbol of the feature."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from oracle import safe_oracle as orc
import strata_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0xDEADBEEF12345678


@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 300])
def test_one_stratum_is_the_device_stream(k):
    rng = np.random.default_rng(k)
    n = k + k // 3 + 2
    movable = np.zeros(n, dtype=np.uint8)
    movable[rng.choice(n, k, replace=False)] = 1                              # rows that do not move lie between the others
    labels = rng.integers(-50, 50, size=n)
    labels[movable == 1] = 31                                                 # one stratum, whatever its label
    np.testing.assert_array_equal(sr.strata_tables(n, movable, labels, 5, KEY), orc.device_stream_tables(n, movable, 5, KEY))


def test_rows_are_permutations_inside_the_strata():
    rng = np.random.default_rng(2)
    n = 400
    movable = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    labels = rng.choice([7, 3, 900, 12, 55], size=n, p=[0.5, 0.3, 0.1, 0.05, 0.05])
    t = sr.strata_tables(n, movable, labels, 25, KEY)
    assert (np.sort(t, axis=1) == np.arange(n)).all()
    assert (labels[t] == labels)[:, movable == 1].all()
    assert (t[:, movable == 0] == np.flatnonzero(movable == 0)).all()
    assert (t != np.arange(n)).any(axis=1).all() and len(np.unique(t, axis=0)) == 25
    # the partition is what counts, not the labels' values: relabelling in the same order gives the same tables
    relabelled = np.searchsorted(np.unique(labels), labels) * 3 + 1
    np.testing.assert_array_equal(sr.strata_tables(n, movable, relabelled, 4, KEY), t[:4])


def test_uniform_and_independent_over_strata():
    """Strata of 3, 2 and 1 rows: 3! 2! 1! = 12 joint arrangements, each with probability 1 / 12 when every stratum is shuffled
    uniformly and the strata independently.  P = 12000: every count within 5 sigma of P / 12, sigma = sqrt(P 11 / 144).  (The
    key is fixed; the restatement's own counts lie within 2.3 sigma.)"""
    P = 12000
    labels = np.array([4, 9, 4, 0, 9, 4])
    t = sr.strata_tables(6, np.ones(6, dtype=np.uint8), labels, P, 1)
    assert (labels[t] == labels).all()
    counts = np.unique(t, axis=0, return_counts=True)[1]
    assert len(counts) == 12
    sigma = np.sqrt(P * 11 / 144.0)
    print('largest deviation: %.2f sigma' % (np.abs(counts - P / 12.0).max() / sigma))
    assert (np.abs(counts - P / 12.0) <= 5 * sigma).all(), counts


def test_neighborhood_size_binning_by_hand():
    """Sizes 3 1 3 2 1 3 2 -> ascending (size, node): nodes 1 4 | 3 6 | 0 2 5; array_split of 7 into 3 gives groups of 3, 2, 2:
    {1, 4, 3}, {6, 0}, {2, 5} -- the tie between nodes 3 and 6 (size 2) and among 0, 2, 5 (size 3) is cut by node index."""
    from safepy_amd import safe
    sizes = np.array([3, 1, 3, 2, 1, 3, 2])
    want = [1, 0, 2, 0, 0, 2, 1]
    assert sr.neighborhood_size_strata(sizes, 3).tolist() == want
    got = safe._neighborhood_size_strata(sizes, 3)
    assert got.dtype == np.int32 and got.tolist() == want
    assert safe._neighborhood_size_strata(sizes, 1).tolist() == [0] * 7
    assert safe._neighborhood_size_strata(sizes, 7).tolist() == [4, 0, 5, 2, 1, 6, 3]          # N bins: singletons
    rng = np.random.default_rng(0)
    for n, bins in [(50, 10), (53, 10), (9, 4), (5, 8)]:
        sizes = rng.integers(1, 6, size=n)                                    # many ties
        np.testing.assert_array_equal(safe._neighborhood_size_strata(sizes, bins), sr.neighborhood_size_strata(sizes, bins))


def test_labels_are_factorised():
    from safepy_amd import safe
    assert safe._factorise_strata(['b', 'a', 'c', 'a'], 4).tolist() == [1, 0, 2, 0]
    assert safe._factorise_strata([10, -3, 10, 7], 4).tolist() == [2, 0, 2, 1]
    assert safe._factorise_strata(np.array([1.5, 0.5]), 2).dtype == np.int32
    for bad in (['a', None, 'b'], [1.0, np.nan, 2.0], np.array([1, 2, None], dtype=object), [1, 2], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            safe._factorise_strata(bad, 3)


def test_validate_config_ini_and_pickle(tmp_path):
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    assert sf.permutation_strata is None and sf.permutation_strata_bins == 10
    assert sf.permutation_strata_resolved is None and sf.permutation_strata_sizes is None
    for bad in ('degree', 3, [[1, 2], [3, 4]]):
        sf.permutation_strata = bad
        with pytest.raises(ValueError, match='permutation_strata'):
            sf.validate_config()
        assert sf.permutation_strata is None                                  # restored
    for ok in ('neighborhood_size', [0, 1, 0], np.arange(4), None):
        sf.permutation_strata = ok
        sf.validate_config()
    for bad in (0, -2, 2.5, True, '10', None):
        sf.permutation_strata_bins = bad
        with pytest.raises(ValueError, match='permutation_strata_bins'):
            sf.validate_config()
        assert sf.permutation_strata_bins == 10
    sf.permutation_strata_bins = np.int64(4)
    sf.validate_config()

    ini = tmp_path / 'strata.ini'
    ini.write_text('[Analysis parameters]\npermutationStrata = neighborhood_size\npermutationStrataBins = 7\n')
    sf = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert sf.permutation_strata == 'neighborhood_size' and sf.permutation_strata_bins == 7
    ini.write_text('[Analysis parameters]\npermutationStrata =\n')
    sf = safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)
    assert sf.permutation_strata is None and sf.permutation_strata_bins == 10
    for text in ('permutationStrata = degree\n', 'permutationStrataBins = 0\n', 'permutationStrataBins = many\n'):
        ini.write_text('[Analysis parameters]\n' + text)
        with pytest.raises(ValueError, match='permutation_strata'):
            safepy_amd.SAFE(path_to_ini_file=str(ini), verbose=False)

    sf = safepy_amd.SAFE(verbose=False)
    sf.permutation_strata, sf.permutation_strata_bins = np.array(['x', 'y', 'x']), 3
    back = pickle.loads(pickle.dumps(sf))
    assert back.permutation_strata.tolist() == ['x', 'y', 'x'] and back.permutation_strata_bins == 3
    state = sf.__getstate__()
    for name in ('permutation_strata', 'permutation_strata_bins', 'permutation_strata_resolved', 'permutation_strata_sizes'):
        del state[name]                                                       # an object pickled before the settings existed
    old = safepy_amd.SAFE.__new__(safepy_amd.SAFE)
    old.__setstate__(state)
    assert old.permutation_strata is None and old.permutation_strata_bins == 10
    assert old.permutation_strata_resolved is None and old.permutation_strata_sizes is None
    old.validate_config()


def test_refusals_before_any_device_work():
    """how = 'analytic' and how = 'hypergeometric' with strata, labels that do not fit the nodes and 'neighborhood_size' without
    neighborhoods are refused before a device is touched (this test has none) and leave the results as they were."""
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    sf.node2attribute = np.zeros((5, 2))
    marks = {name: object() for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')}
    for name, mark in marks.items():
        setattr(sf, name, mark)
    labels = [0, 1, 0, 1, 0]
    for kwargs, message in [(dict(how='analytic', permutation_strata=labels), 'analytic'),
                            (dict(how='hypergeometric', permutation_strata=labels), "how = 'randomization'"),
                            (dict(how='randomization', permutation_strata=labels[:4]), 'expected length 5'),
                            (dict(how='randomization', permutation_strata=[0, None, 1, 1, 0]), 'missing labels'),
                            (dict(how='randomization', permutation_strata='neighborhood_size'), 'define_neighborhoods'),
                            (dict(how='randomization', permutation_strata='degree'), 'not a valid setting'),
                            (dict(how='randomization', permutation_strata=labels, permutation_strata_bins=0), 'permutation_strata_bins')]:
        with pytest.raises(ValueError, match=message):
            sf.compute_pvalues(**kwargs)
        for name, mark in marks.items():
            assert getattr(sf, name) is mark, (kwargs, name)
        assert sf.permutation_strata_resolved is None and sf.permutation_strata_sizes is None
        sf.permutation_strata, sf.permutation_strata_bins = None, 10
    with pytest.raises(ValueError, match='define_neighborhoods'):             # the randomization entry point called directly
        sf.compute_pvalues_by_randomization(permutation_strata='neighborhood_size')
    assert all(getattr(sf, name) is mark for name, mark in marks.items())


def test_symbol_is_declared_bound_and_exported():
    from safepy_amd import _lib, backend
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    found = re.search(r'\bint\s+safe_perms_create_device_strata\s*\(([^)]*)\)', code)
    assert found and len(found.group(1).split(',')) == 7
    assert 'const int32_t *stratum_host' in found.group(1)
    res, args = _lib.PROTOTYPES['safe_perms_create_device_strata']
    assert res is ctypes.c_int and len(args) == 7 and args[5] is ctypes.c_uint64
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'safe_perms_create_device_strata')
    assert hasattr(backend.Permutations, 'stratified')
    # NULL arguments are refused before a device is touched, and *out is cleared
    out = ctypes.c_void_p(1)
    assert _lib.lib.safe_perms_create_device_strata(None, 4, None, None, 1, ctypes.c_uint64(0), ctypes.byref(out)) == _lib.E_INVALID
    assert out.value is None and b'NULL argument' in _lib.lib.safe_last_error()
