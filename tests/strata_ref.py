"""NumPy restatement of the restricted permutation stream (safe_perms_create_device_strata, include/safe_hip.h) and of the
'neighborhood_size' binning of SAFE.permutation_strata, for the tests.  Checker only: nothing here is imported by the package.

The stream: the movable rows are listed stratum by stratum (strata in ascending label order, rows ascending inside a stratum);
row q of the table shuffles every stratum's element list on its own with the device stream's algorithm
(oracle.safe_oracle.device_stream_tables) -- element index e and step i local to the stratum, the stratum's rank s in word 2 of
every Philox counter, (s << 16) | tag.  The restatement is vectorised over the elements of all strata (one Philox evaluation
per element, no word cache), so it shares no structure with the kernel's lane and wave forms."""
import numpy as np

from oracle.safe_oracle import _philox4x32_10

_U = np.uint64


def partition(movable, strata):
    """(order, rank, offs): the movable rows stratum by stratum, the stratum rank of every entry of that list, and the starts
    of the strata in it.  `strata`: integer labels, read where `movable` is set."""
    mov = np.flatnonzero(np.asarray(movable).astype(bool))
    labels = np.asarray(strata)[mov]
    rank = np.unique(labels, return_inverse=True)[1].reshape(-1) if len(mov) else np.zeros(0, dtype=np.int64)
    by_stratum = np.argsort(rank, kind='stable')
    order, rank = mov[by_stratum], rank[by_stratum].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(np.bincount(rank))]).astype(np.int64) if len(mov) else np.zeros(1, dtype=np.int64)
    return order, rank, offs


def _fallback_draw(q, s, b, i, key0, key1):
    rng_range = i + 1
    thresh = ((1 << 32) - rng_range) % rng_range
    r = 0
    while True:
        w = _philox4x32_10([q], [(b << 16) | i], [(s << 16) | 0xFA11], [r], key0, key1)
        for t in range(4):
            m = int(w[t][0]) * rng_range
            if (m & 0xFFFFFFFF) >= thresh:
                return m >> 32
        r += 1


def strata_tables(n, movable, strata, num_permutations, key):
    """int64 [P, n]: the tables safe_perms_create_device_strata generates for `key` (a 64-bit integer)."""
    order, rank, offs = partition(movable, strata)
    k = len(order)
    key0, key1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    out = np.tile(np.arange(n, dtype=np.int64), (num_permutations, 1))
    if k == 0:
        return out
    s = rank.astype(_U)
    e = (np.arange(k, dtype=np.int64) - offs[rank]).astype(_U)               # element index inside its stratum
    idx = np.arange(k)
    zeros = np.zeros(k, dtype=_U)
    for q in range(num_permutations):
        qq = np.full(k, q, dtype=_U)
        words = np.stack(_philox4x32_10(qq, e >> _U(4), (s << _U(16)) | _U(0xB0C7), zeros, key0, key1), axis=1)
        word = words[idx, ((e >> _U(2)) & _U(3)).astype(np.int64)]
        bucket = (word >> (_U(8) * (e & _U(3)))) & _U(63)
        group = (s * _U(64) + bucket).astype(np.int64)
        x = np.argsort(group, kind='stable')                                 # buckets end to end, ascending element order inside
        g = group[x]
        starts = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
        sizes = np.diff(np.concatenate([starts, [k]]))
        step = (idx - np.repeat(starts, sizes)).astype(_U)                   # Fisher-Yates step i of the slot inside its bucket
        gs, gb = _U(1) * (g // 64).astype(_U), (g % 64).astype(_U)
        first = np.stack(_philox4x32_10(qq, (gb << _U(16)) | (step >> _U(2)), (gs << _U(16)) | _U(0x5AFE), zeros, key0, key1), axis=1)
        first = first[idx, (step & _U(3)).astype(np.int64)]
        rng_range = step + _U(1)
        thresh = (_U(1 << 32) - rng_range) % rng_range
        m = first * rng_range
        accepted = ((m & _U(0xFFFFFFFF)) >= thresh).tolist()
        draws = (m >> _U(32)).astype(np.int64).tolist()
        x = x.tolist()
        for lo, size in zip(starts[sizes >= 2].tolist(), sizes[sizes >= 2].tolist()):
            for i in range(size - 1, 0, -1):
                j = draws[lo + i] if accepted[lo + i] else _fallback_draw(q, int(g[lo]) // 64, int(g[lo]) % 64, i, key0, key1)
                x[lo + i], x[lo + j] = x[lo + j], x[lo + i]
        out[q, order] = order[np.array(x, dtype=np.int64)]
    return out


def neighborhood_size_strata(sizes, bins):
    """int64 [N]: the stratum of every node under permutation_strata='neighborhood_size' -- the nodes in ascending
    (neighborhood size, node index) order, cut into `bins` groups the way np.array_split cuts N items."""
    sizes = np.asarray(sizes)
    n = len(sizes)
    by_size = sorted(range(n), key=lambda i: (int(sizes[i]), i))
    long_groups, short = n % bins, n // bins                                 # np.array_split: the first N % bins groups hold one more
    out = np.empty(n, dtype=np.int64)
    at = 0
    for b in range(bins):
        width = short + (1 if b < long_groups else 0)
        for i in by_size[at:at + width]:
            out[i] = b
        at += width
    return out
