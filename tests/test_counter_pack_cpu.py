"""The reference helpers of the counter epilogue tests (tests/counter_ref.py) themselves: the 20-bit exchange form against
bytes worked out by hand and as a round trip, the arithmetic from counter pairs to the matrices against the oracle.  CPU."""
import numpy as np
import pytest

import counter_ref as cr
from oracle import safe_oracle as orc


def _u32(less, greater):
    return (np.asarray(less, dtype=np.uint32) << np.uint32(16)) | np.asarray(greater, dtype=np.uint32)


def test_pack20_bytes_by_hand():
    """One column of eight positions = twenty bytes.  A pair is #less << 10 | #greater; positions 2 i (low 20 bits) and
    2 i + 1 (high 20 bits) make 40 bits, low 32 in word i, high 8 in byte i behind the four words:
      (1, 2), (512, 513):        0x00402 | 0x80201 << 20 = 0x80_20100402
      (1023, 1023), (0, 0):      0xFFFFF                 = 0x00_000FFFFF
      (0, 0), (1023, 1023):      0xFFFFF << 20           = 0xFF_FFF00000
      (5, 7), (341, 682):        0x01407 | 0x556AA << 20 = 0x55_6AA01407
    The first two groups alone are the ten bytes of four positions: words 0-1 and side bytes 0-1."""
    less = [1, 512, 1023, 0, 0, 1023, 5, 341]
    greater = [2, 513, 1023, 0, 0, 1023, 7, 682]
    want = bytes([0x02, 0x04, 0x10, 0x20, 0xFF, 0xFF, 0x0F, 0x00, 0x00, 0x00, 0xF0, 0xFF, 0x07, 0x14, 0xA0, 0x6A,
                  0x80, 0x00, 0xFF, 0x55])
    got = cr.pack20(_u32(less, greater), 8, 1)
    assert got.dtype == np.uint32 and got.shape == (5,)
    assert got.astype('<u4').tobytes() == want
    np.testing.assert_array_equal(cr.unpack20(np.frombuffer(want, dtype='<u4'), 8, 1), _u32(less, greater))


@pytest.mark.parametrize('n_pad,cols', [(8, 1), (64, 3), (256, 5)])
def test_pack20_round_trip(n_pad, cols):
    rng = np.random.default_rng(n_pad + cols)
    slabs = [np.zeros(cols * n_pad, dtype=np.uint32), np.full(cols * n_pad, 0x03FF03FF, dtype=np.uint32),
             _u32(rng.integers(0, 1024, cols * n_pad), rng.integers(0, 1024, cols * n_pad))]
    for pos in (0, 1, n_pad - 2, n_pad - 1, (cols - 1) * n_pad + 3):               # one bit in one field of one position
        for bit in list(range(10)) + list(range(16, 26)):
            one = np.zeros(cols * n_pad, dtype=np.uint32)
            one[pos] = np.uint32(1) << np.uint32(bit)
            slabs.append(one)
    for x in slabs:
        words = cr.pack20(x, n_pad, cols)
        assert words.shape == (cols * n_pad // 8 * 5,) and words.dtype == np.uint32
        np.testing.assert_array_equal(cr.unpack20(words, n_pad, cols), x)
    # a single set bit stays a single set bit: 20 * (pos & 1) + (10 for #less) + k of the 40-bit group pos / 2
    for pos, bit in ((0, 0), (1, 9), (1, 25), (n_pad - 1, 16), (n_pad - 2, 25)):
        one = np.zeros(n_pad, dtype=np.uint32)
        one[pos] = np.uint32(1) << np.uint32(bit)
        words = cr.pack20(one, n_pad, 1)
        at = 20 * (pos & 1) + (bit if bit < 16 else bit - 16 + 10)
        raw = words.astype('<u4').tobytes()
        group = int.from_bytes(raw[4 * (pos // 2):4 * (pos // 2) + 4], 'little') | raw[4 * (n_pad // 2) + pos // 2] << 32
        assert group == 1 << at and sum(bin(b).count('1') for b in raw) == 1


def test_pack20_refuses_counts_above_1023():
    with pytest.raises(AssertionError):
        cr.pack20(_u32([1024], [0]).repeat(8), 8, 1)


@pytest.mark.parametrize('sign', cr.SIGNS)
@pytest.mark.parametrize('score,binary', [('sum', True), ('sum', False), ('z-score', False)])
def test_outputs_from_pairs_equal_the_oracle(sign, score, binary):
    """The oracle's compute_pvalues on a tiny seeded case == outputs_from_pairs on the pairs its run_permutations counts
    give (#less = P - #>=, #greater = P - #<=), wherever the observed score is a number."""
    rng = np.random.default_rng(11)
    n, m, P, seed = 40, 9, 37, 5
    xy = rng.uniform(size=(n, 2))
    a = orc.neighborhoods_euclidean(xy, 0.25)
    b = (rng.uniform(size=(n, m)) < 0.3).astype(np.float64) if binary else rng.normal(size=(n, m))
    b[rng.choice(n, 3, replace=False)] = np.nan
    for thr in (0.05, 0.1):
        want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', neighborhood_score_type=score, num_permutations=P,
                                   random_seed=seed, attribute_sign=sign, enrichment_threshold=thr)
        cn, cp = orc.run_permutations(a, b.copy(), score, P, seed)
        ok = ~np.isnan(want['ns'])
        assert ok.sum() > n * m // 2
        got = cr.outputs_from_pairs(P - cp, P - cn, P, sign, thr)
        for k in cr.NAMES:
            np.testing.assert_array_equal(got[k][ok], want[k][ok], err_msg=k)
    # the table the library is handed holds the same values: tab[#>=] is the 'highest' NES
    np.testing.assert_array_equal(cr.nes_table(P)[cp[ok].astype(np.int64)], cr.outputs_from_pairs(P - cp, P - cn, P, 'highest', 0.05)['nes'][ok])


@pytest.mark.parametrize('P', [1, 2, 255, 511, 512, 1023, 1024, 2560, 65535, 100000])
def test_designed_pairs_are_valid_and_reach_every_bit(P):
    less, greater = cr.designed_pairs(P)
    assert (less + greater <= P).all() and less.min() == 0 and greater.min() == 0 and less.max() == P and greater.max() == P
    for k in range(P.bit_length()):
        for field in (less, greater):
            assert (1 << k) in field and (1 << k) - 1 in field
    rng = np.random.default_rng(P)
    parity = np.arange(50) & 1
    l, g = cr.designed_matrix(P, 50, 7, parity, rng)
    for par in (0, 1):
        have = set(zip(l[parity == par].ravel().tolist(), g[parity == par].ravel().tolist()))
        assert set(zip(less.tolist(), greater.tolist())) <= have
    if P <= 65535:                                                        # (the u32 form's 16-bit fields)
        s = cr.slab_u32(l, g, np.arange(50) + 3, 56).reshape(7, 56)
        assert (s[:, :3] == 0xFFFFFFFF).all() and (s[:, 53:] == 0xFFFFFFFF).all()
        np.testing.assert_array_equal(s[:, 3:53] >> 16, l.T)
        np.testing.assert_array_equal(s[:, 3:53] & 0xFFFF, g.T)
