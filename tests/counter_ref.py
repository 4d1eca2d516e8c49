"""Plain NumPy restatements for the counter epilogue tests (tests/test_gpu_counter_epilogue.py, test_counter_pack_cpu.py):
the reference's arithmetic from permutation counter pairs to its matrices (safepy/safe.py:532-554, 468-472), the 20-bit
exchange form of include/safe_hip.h, and the designed counter pairs the GPU tests feed to the consumers.  Nothing here
calls the library."""
import numpy as np

SIGNS = ('highest', 'lowest', 'both')
NAMES = ('pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary')


def nes_table(num_permutations):
    """tab[k] = -log10(k / P), tab[0] = -log10(1 / P): what the reference's np.log10 gives for every possible count
    (safe.py:546-547) -- the nes_table_host argument of the library."""
    P = int(num_permutations)
    p = np.arange(P + 1, dtype=np.float64) / P
    return np.ascontiguousarray(-np.log10(np.where(p == 0, 1 / P, p)))


def outputs_from_pairs(less, greater, P, sign, threshold):
    """{pvalues_neg, pvalues_pos, nes, nes_binary} from #(S_p < S_obs) and #(S_p > S_obs) out of P permutations, operation
    by operation as the reference: counts (safe_extras.py:65-66: #<= = P - #greater, #>= = P - #less), counts / P
    (safe.py:532-533), zero p-values as 1 / P inside -log10 (546-547), the sign (549-554), the binarisation (468-472)."""
    P = int(P)
    counts_neg = (P - np.asarray(greater, dtype=np.int64)).astype(np.float64)
    counts_pos = (P - np.asarray(less, dtype=np.int64)).astype(np.float64)
    pvalues_neg = counts_neg / P
    pvalues_pos = counts_pos / P
    nes_pos = -np.log10(np.where(pvalues_pos == 0, 1 / P, pvalues_pos))
    nes_neg = -np.log10(np.where(pvalues_neg == 0, 1 / P, pvalues_neg))
    if sign == 'highest':
        nes = nes_pos
    elif sign == 'lowest':
        nes = nes_neg
    else:
        nes = nes_pos - nes_neg
    idx = ~np.isnan(nes)
    nes_binary = np.zeros(nes.shape)
    nes_binary[idx] = np.abs(nes[idx]) > -np.log10(threshold)
    return {'pvalues_neg': pvalues_neg, 'pvalues_pos': pvalues_pos, 'nes': nes, 'nes_binary': nes_binary}


# ---- the 20-bit exchange form (safe_hip.h, safe_export_packed_chunk_narrow) -----------------------------------------
# u32 form: [cols][n_pad] counters (#less << 16 | #greater).  Narrow form: a pair is #less << 10 | #greater (20 bits); the
# pairs of positions 2 i and 2 i + 1 share 40 bits (the even position low); a column is n_pad / 2 words -- the low 32 bits
# of every 40 -- followed by n_pad / 2 bytes -- the high 8 --, 5 n_pad / 8 words in all.

def pack20(u32_slab, n_pad, cols):
    """u32 counters [cols * n_pad], both fields <= 1023 -> u32 words [cols * 5 n_pad / 8] of the narrow form."""
    assert n_pad % 8 == 0
    v = np.asarray(u32_slab, dtype=np.uint32).reshape(cols, n_pad).astype(np.uint64)
    less, greater = v >> np.uint64(16), v & np.uint64(0xFFFF)
    assert less.max(initial=0) <= 1023 and greater.max(initial=0) <= 1023, 'a 10-bit field holds at most 1023'
    pair = (less << np.uint64(10)) | greater
    x = pair[:, 0::2] | (pair[:, 1::2] << np.uint64(20))                  # 40 bits per two positions
    out = np.zeros((cols, n_pad // 8 * 5), dtype=np.uint32)
    out[:, :n_pad // 2] = (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    side = np.ascontiguousarray((x >> np.uint64(32)).astype(np.uint8))
    out[:, n_pad // 2:] = side.view('<u4')
    return out.reshape(-1)


def unpack20(words, n_pad, cols):
    """The inverse: narrow words [cols * 5 n_pad / 8] -> u32 counters [cols * n_pad]."""
    assert n_pad % 8 == 0
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(cols, n_pad // 8 * 5))
    low = w[:, :n_pad // 2].astype(np.uint64)
    side = np.ascontiguousarray(w[:, n_pad // 2:]).astype('<u4').view(np.uint8).reshape(cols, n_pad // 2).astype(np.uint64)
    x = low | (side << np.uint64(32))
    pair = np.empty((cols, n_pad), dtype=np.uint64)
    pair[:, 0::2] = x & np.uint64(0xFFFFF)
    pair[:, 1::2] = x >> np.uint64(20)
    out = ((pair >> np.uint64(10)) << np.uint64(16)) | (pair & np.uint64(0x3FF))
    return out.astype(np.uint32).reshape(-1)


# ---- designed counter pairs -------------------------------------------------------------------------------------------

def designed_pairs(P, thresholds=(0.05, 0.1)):
    """The (less, greater) pairs every case contains, all with less + greater <= P: the corners, 2^k and 2^k - 1 in each
    field alone for every k a count up to P has, and the counts whose p-value is exactly an enrichment threshold where P
    admits one (|NES| == -log10(threshold) is NOT enriched: the comparison is strict, safe.py:470)."""
    P = int(P)
    pairs = [(0, 0), (P, 0), (0, P), (1, P - 1), (P - 1, 1), (P // 2, P - P // 2)]
    for k in range(P.bit_length()):
        for v in (1 << k, (1 << k) - 1):
            if v <= P:
                pairs += [(v, 0), (0, v)]
    for t in thresholds:
        k = int(round(P * t))                                             # count k: p = k / P, the count's field P - k
        for kk in (k - 1, k, k + 1):
            if 0 <= kk <= P:
                pairs += [(P - kk, 0), (0, P - kk)]
    a = np.array(pairs, dtype=np.int64)
    assert (a >= 0).all() and (a.sum(axis=1) <= P).all()
    return a[:, 0], a[:, 1]


def designed_matrix(P, n, m, pos_parity, rng):
    """less, greater as int64 [n, m]: random valid pairs everywhere, then the designed pairs twice, once in cells whose
    counter position is even and once in cells whose position is odd (pos_parity[row] = position & 1; the narrow form packs
    the two parities into different bits), column after column from column 0 on, as far as the matrix has room."""
    P = int(P)
    less = rng.integers(0, P + 1, size=(n, m))
    greater = rng.integers(0, P - less + 1)
    dl, dg = designed_pairs(P)
    for parity in (0, 1):
        rows = np.nonzero(np.asarray(pos_parity) == parity)[0]
        cells = [(r, c) for c in range(min(m, len(dl) // max(len(rows), 1) + 1)) for r in rows][:len(dl)]
        for (r, c), l, g in zip(cells, dl, dg):
            less[r, c], greater[r, c] = l, g
    assert (less + greater <= P).all() and less.min() >= 0 and greater.min() >= 0
    return less, greater


def slab_u32(less, greater, pos_of_row, n_pad, poison=0xFFFFFFFF):
    """The u32 counter slab [m * n_pad] of pair matrices [n, m]: row r at position pos_of_row[r] of every column, every
    other (padding) position poisoned."""
    n, m = less.shape
    slab = np.full((m, n_pad), poison, dtype=np.uint32)
    slab[:, np.asarray(pos_of_row)] = ((less.astype(np.uint32) << np.uint32(16)) | greater.astype(np.uint32)).T
    return slab.reshape(-1)
