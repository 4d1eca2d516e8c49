"""Sparse attribute input, the parts that need no device: the new symbol in the header and the binding, the host-side
canonicalisation of backend.Attributes.from_sparse, and the refusals of the consumers that need a dense matrix."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_versioned():
    from safepy_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(r'\bint\s+safe_attr_create_csc_host\s*\(', code)
    assert '#define SAFE_HIP_ABI_VERSION 9' in header
    assert _lib.ABI_VERSION == 9 and _lib.lib.safe_abi_version() == 9
    res, args = _lib.PROTOTYPES['safe_attr_create_csc_host']
    assert len(args) == 10                                   # ctx, n, m, nnz, indptr, indices, values, dtype, missing_rows, out
    assert hasattr(_lib.lib, 'safe_attr_create_csc_host')


def small():
    """4 x 3, column 1 given twice over (duplicates), rows out of order."""
    rows = np.array([3, 0, 2, 2, 1, 3, 0])
    cols = np.array([0, 0, 1, 1, 1, 2, 2])
    vals = np.array([1.0, 1.0, 0.25, 0.75, 1.0, 1.0, 1.0])
    return sp.coo_matrix((vals, (rows, cols)), shape=(4, 3))


@pytest.mark.parametrize('form', ['coo', 'csr', 'csc', 'lil', 'csc_array'])
def test_canonical_csc_against_toarray(form):
    from safepy_amd.backend import Attributes
    a = small()
    a = {'coo': a, 'csr': a.tocsr(), 'csc': a.tocsc(), 'lil': a.tolil(), 'csc_array': sp.csc_array(a.tocsc())}[form]
    before = a.toarray().copy()
    n, m, indptr, indices, values, _ = Attributes.canonical_csc(a)
    assert (n, m) == (4, 3)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and indptr.flags.c_contiguous and indices.flags.c_contiguous
    assert indptr.tolist() == [0, 2, 4, 6] and indices.tolist() == [0, 3, 1, 2, 0, 3]          # summed, sorted
    assert values is None                                    # 0.25 + 0.75 = 1: every stored value is 1
    dense = np.zeros((n, m))
    for j in range(m):
        dense[indices[indptr[j]:indptr[j + 1]], j] = 1
    assert np.array_equal(dense, before)
    assert np.array_equal(a.toarray(), before), 'canonical_csc changed its input'


def test_canonical_csc_values_and_dtypes():
    from safepy_amd.backend import Attributes
    base = small().tocsc()
    base.sum_duplicates()
    # bool / integer data of ones: no values travel
    for dtype in (bool, np.int8, np.int64, np.float32, np.float64):
        assert Attributes.canonical_csc(base.astype(dtype))[4] is None, dtype
    # integer data with another value: promoted to f64
    two = base.astype(np.int32)
    two.data[1] = 2
    v = Attributes.canonical_csc(two)[4]
    assert v.dtype == np.float64 and v.tolist() == two.data.tolist()
    # f32 stays f32; a stored zero and a stored NaN are kept as stored entries
    q = base.astype(np.float32)
    q.data[0], q.data[2] = 0.0, np.nan
    n, m, indptr, indices, v, _ = Attributes.canonical_csc(q)
    assert v.dtype == np.float32 and indices.shape[0] == base.nnz
    assert v[0] == 0.0 and np.isnan(v[2])
    # duplicates meet in the input's own dtype, as in toarray(): True + True is True
    dup = sp.coo_matrix((np.array([True, True]), (np.array([1, 1]), np.array([0, 0]))), shape=(3, 1))
    assert dup.toarray().tolist() == [[False], [True], [False]]
    _, _, _, indices, values, _ = Attributes.canonical_csc(dup)
    assert indices.tolist() == [1] and values is None
    with pytest.raises(TypeError):
        Attributes.canonical_csc(np.zeros((3, 3)))


def test_load_attributes_refusals():
    """What SAFE.load_attributes and compute_pvalues refuse before any device work (no context is created)."""
    import safepy_amd
    sf = safepy_amd.SAFE(verbose=False)
    with pytest.raises(TypeError) as err:
        sf.load_attributes(attribute_file=np.zeros((4, 3)), missing_rows=np.zeros(4))
    assert 'missing_rows' in str(err.value) and 'sparse' in str(err.value)
    with pytest.raises(ValueError) as err:
        sf.load_attributes(attribute_file=small().tocsc(), missing_rows=np.zeros(5))
    assert 'missing_rows' in str(err.value)
    a = small().tocsc()
    sf.load_attributes(attribute_file=a, missing_rows=[0, 1, 0, 0])
    assert sf.node2attribute is a and sf._missing_rows.tolist() == [0, 1, 0, 0]
    assert sf.attributes['name'].tolist() == ['0', '1', '2']
    # background='network' needs the stored values in one array (.data): LIL has none
    sf.load_attributes(attribute_file=small().tolil())
    with pytest.raises(TypeError) as err:
        sf.compute_pvalues(background='network')
    assert '.tocsc()' in str(err.value)
