"""attribute_transform = 'rank' where no GPU exists: the NumPy restatement of rank.hip's key transform and of
(less + leq + 1) / 2 (tests/rank_ref.py) against scipy.stats.rankdata on the bits, over the GPU test's own case list; the
setting's validation and pickling; the new symbols; the refusal of the hypergeometric route, which needs no device."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import rank_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keys_order_like_the_values():
    v = np.array([-np.inf, -1e300, -1.0, np.nextafter(-1.0, 0), -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308, 1.0,
                  np.nextafter(1.0, 2), 1e300, np.inf, np.nan])
    k = rr.keys(v[:, None])[:, 0]
    assert k[5] == k[6]                                        # -0.0 ties with +0.0
    rest = np.delete(k, 5)
    assert (np.diff(rest.astype(object)) > 0).all()            # strictly ascending, NaN (all ones) last
    assert k[-1] == rr.NAN_KEY and k[-2] < rr.NAN_KEY
    f = np.array([1e-45, np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))], dtype=np.float32)
    kf = rr.keys(f[:, None])[:, 0]
    assert kf[0] < kf[1] < kf[2] and kf[0] > rr.keys(np.zeros((1, 1)))[0, 0]


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('n', rr.shapes_n())
def test_restatement_equals_scipy_on_the_designed_columns(n, dtype):
    b = rr.designed(n, dtype)
    got, want = rr.midranks(b), rr.want_cached('designed', n, dtype) if dtype == 'float32' else rr.want_cached('designed', n)
    bad = [name for j, name in enumerate(rr.column_kinds(n, dtype)) if not np.array_equal(got[:, j], want[:, j], equal_nan=True)]
    assert not bad and rr.same(got, want), (n, dtype, bad)
    live = ~np.isnan(want)
    assert (want[live] * 2 == np.round(want[live] * 2)).all() and np.array_equal(np.isnan(want), np.isnan(b))


def test_restatement_equals_scipy_on_the_other_cases():
    assert rr.same(rr.midranks(rr.big()), rr.want_cached('big'))
    for n, m in ((1, 1), (1, 65), (130, 63), (130, 129)):
        b = rr.tiled(n, m, 'float32', 'C')
        assert rr.same(rr.midranks(b), rr.want(b))
    assert rr.want(np.empty((5, 0))).shape == rr.midranks(np.empty((5, 0))).shape == (5, 0)


def test_the_case_list_covers_what_it_names():
    t = rr.chunk()
    assert t >= 512 and t & (t - 1) == 0
    n = 3 * t + 7
    cols = rr.column_kinds(n)
    assert len(cols) == 16
    assert 5e-324 in np.abs(cols['subnormals']) and (cols['subnormals'] == 0).any()
    z = cols['signed_zeros']
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    assert np.isinf(cols['infinities']).any() and (cols['infinities'] == -np.inf).any()
    run = cols['run_on_edges']
    for edge in (t, 2 * t, 3 * t):
        assert (run[edge - 3:edge + 3] == 0.125).all()
    u = np.unique(cols['one_ulp_apart'])
    assert len(u) == 8 and (u < 0).sum() == 4
    c = cols['f32_colliders']
    assert len(np.unique(c)) == 4 and len(np.unique(c.astype(np.float32))) == 1
    c = rr.column_kinds(n, 'float32')['f16_colliders']
    assert len(np.unique(c)) == 4 and len(np.unique(c.astype(np.float16))) == 1
    assert np.isnan(cols['all_nan']).all() and (~np.isnan(cols['single_value'])).sum() == 1
    for pct in (1, 50, 99):
        assert abs(np.isnan(cols['nan_%d' % pct]).mean() - pct / 100.0) < 0.02
    ones = cols['zero_one'].sum()
    assert ones > 1000 and n - ones > 1000                      # ties of thousands across the chunk edges
    assert np.isnan(rr.designed(n)[n // 2]).all()               # the whole-NaN row


def test_symbols_and_abi():
    from safepy_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    assert re.search(r'int safe_attr_rank\(safe_attr \*src, safe_attr \*\*out\);', header)
    assert re.search(r'#define SAFE_HIP_ABI_VERSION 9\b', header) and _lib.ABI_VERSION == 9 and _lib.lib.safe_abi_version() == 9
    assert int(re.search(r'#define SAFE_RANK_CHUNK (\d+)', header).group(1)) == _lib.RANK_CHUNK
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('safe_attr_rank', 'safe_last_rank_stats'):
        assert hasattr(raw, name) and _lib.PROTOTYPES[name][0] is ctypes.c_int, name
    assert len(_lib.PROTOTYPES['safe_attr_rank'][1]) == 2 and len(_lib.PROTOTYPES['safe_last_rank_stats'][1]) == 4
    # NULL arguments: the usual code, nothing created, no device needed
    h = ctypes.c_void_p()
    assert _lib.lib.safe_attr_rank(None, ctypes.byref(h)) == _lib.E_INVALID and not h.value
    assert b'NULL' in _lib.lib.safe_last_error()
    from safepy_amd import backend as be
    assert be.AttributeMatrix is be.Attributes and callable(be.AttributeMatrix.rank)


def make_safe(**kwargs):
    import safepy_amd
    return safepy_amd.SAFE(verbose=False, **kwargs)


def test_setting_is_validated_and_pickles():
    sf = make_safe()
    assert sf.attribute_transform == 'none'
    sf.attribute_transform = 'rank'
    sf.validate_config()
    back = pickle.loads(pickle.dumps(sf))
    assert back.attribute_transform == 'rank'
    sf.attribute_transform = 'ranks'
    with pytest.raises(ValueError, match='attribute_transform'):
        sf.validate_config()
    assert sf.attribute_transform == 'none'                     # the default is restored
    # an object pickled before the setting existed
    state = sf.__getstate__()
    del state['attribute_transform']
    old = sf.__class__.__new__(sf.__class__)
    old.__setstate__(state)
    assert old.attribute_transform == 'none'
    del old.__dict__['attribute_transform']
    old.validate_config()                                       # (the getattr guard)


def test_bad_keyword_is_refused_before_any_device_work():
    sf = make_safe()
    sf.node2attribute = np.zeros((4, 2))
    with pytest.raises(ValueError, match='attribute_transform'):
        sf.compute_pvalues(attribute_transform='midrank')
    assert sf.attribute_transform == 'none' and sf.ns is None and sf.pvalues_pos is None


def test_hypergeometric_route_is_refused_without_a_device():
    sf = make_safe()
    sf.node2attribute = (np.arange(8).reshape(4, 2) % 2).astype(np.float64)
    with pytest.raises(ValueError, match='ranks are not counts'):
        sf.compute_pvalues(how='hypergeometric', attribute_transform='rank')
    for name in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):
        assert getattr(sf, name) is None, name
