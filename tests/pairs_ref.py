"""Host restatement of SAFE.enriched_pairs' selection and ordering (NumPy only): which cells of a result matrix are selected
and in which order the three arrays of a CSR / CSC / COO matrix list them.  tests/test_enriched_pairs_cpu.py holds it to
SciPy's own constructors; the GPU tests compare the device's arrays with it exactly."""
import numpy as np

MODE_POSITIVE_NONZERO, MODE_BOTH, MODE_POSITIVE, MODE_NEGATIVE = 0, 1, 2, 3
SIDE_MODES = {'both': MODE_BOTH, 'positive': MODE_POSITIVE, 'negative': MODE_NEGATIVE}


def selected(sel, mode, threshold=0.0):
    """bool [n, m]: mode 0 x > 0, 1 |x| > t, 2 x > t, 3 x < -t.  Strict; NaN compares false; -0.0 is not below -0.0."""
    sel = np.asarray(sel, dtype=np.float64)
    t = np.float64(threshold)
    with np.errstate(invalid='ignore'):
        if mode == MODE_POSITIVE_NONZERO:
            return sel > 0
        if mode == MODE_BOTH:
            return np.abs(sel) > t
        if mode == MODE_POSITIVE:
            return sel > t
        if mode == MODE_NEGATIVE:
            return sel < -t
    raise ValueError('mode %r' % (mode,))


def compressed(mask, values, axis):
    """(indptr int32, indices int32, data f64 or None) of the selected cells: axis 0 by row with ascending columns (CSR),
    axis 1 by column with ascending rows (CSC).  data = values at those cells, bit for bit; None without values."""
    mask = np.asarray(mask, dtype=bool)
    if axis == 1:
        mask = mask.T
        values = None if values is None else np.asarray(values).T
    major, minor = np.nonzero(mask)                          # row-major order of the (possibly transposed) mask
    indptr = np.zeros(mask.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(major, minlength=mask.shape[0]), out=indptr[1:])
    data = None if values is None else np.ascontiguousarray(np.asarray(values, dtype=np.float64)[major, minor])
    return indptr.astype(np.int32), minor.astype(np.int32), data


def coo(mask, values):
    """(row int32, col int32, data f64 or None) in row-major order."""
    mask = np.asarray(mask, dtype=bool)
    row, col = np.nonzero(mask)
    data = None if values is None else np.ascontiguousarray(np.asarray(values, dtype=np.float64)[row, col])
    return row.astype(np.int32), col.astype(np.int32), data


def pairs(sel, values, mode, threshold, fmt):
    """The arrays SAFE.enriched_pairs(format=fmt) must hold: (indptr, indices, data) for 'csr' / 'csc', (row, col, data) for
    'coo'; data is None for the pattern-only form (the method then stores int8 ones)."""
    mask = selected(sel, mode, threshold)
    if fmt == 'coo':
        return coo(mask, values)
    return compressed(mask, values, {'csr': 0, 'csc': 1}[fmt])


def bits(a):
    """The bit patterns of a float64 array (NaN payloads and signed zeros compare as what they are)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def special_values(rng, shape, p_special=0.3):
    """float64 `shape` of random 64-bit patterns -- NaNs with payloads, denormals, huge and tiny numbers of both signs --
    with a share p_special of cells drawn from a list of special values (+-0, +-inf, NaNs, denormals, +-1, -log10(0.05))."""
    raw = rng.integers(0, 2 ** 64, size=shape, dtype=np.uint64).view(np.float64)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072009e-308, 1.0, -1.0,
                        -np.log10(0.05), np.log10(0.05)], dtype=np.float64)
    quiet_payload = np.array([0x7FF8000000000123, 0xFFF0000000000001, 0x7FF00000DEADBEEF], dtype=np.uint64).view(np.float64)
    special = np.concatenate([special, quiet_payload])
    pick = rng.random(shape) < p_special
    out = raw.copy()
    out[pick] = special[rng.integers(0, special.shape[0], size=int(pick.sum()))]
    return out
