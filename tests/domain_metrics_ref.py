"""NumPy restatement of the count-to-distance step of the boolean metrics of safe_profile_distances (domains.hip,
metric_distance): what scipy.spatial.distance.pdist (SciPy 1.15) returns for two 0/1 profiles of length n with the
contingency counts ntt, ntf, nft and nff = n - ntt - ntf - nft.

The counts are exact integers far below 2^53, so every sum and product below is exact in f64 and each metric rounds
once, in its division.  What has to be restated is therefore only which quotient SciPy forms and what it returns when
the denominator is zero:

  jaccard         (ntf + nft) / (ntt + ntf + nft)             0 when the denominator is 0
  hamming         (ntf + nft) / n
  dice            (ntf + nft) / (2 ntt + ntf + nft)           0 / 0 = NaN
  rogerstanimoto  2 (ntf + nft) / (n + ntf + nft)
  russellrao      (n - ntt) / n
  sokalmichener   2 (ntf + nft) / (n + ntf + nft)
  sokalsneath     2 (ntf + nft) / (2 (ntf + nft) + ntt)       0 / 0 = NaN
  yule            2 ntf nft / (ntt nff + ntf nft)             0 when ntf nft = 0 (also where ntt nff = 0)

tests/test_domain_metrics_cpu.py holds this table to live SciPy; tests/test_gpu_domain_stage.py holds the kernel to
live SciPy as well, so the table documents the epilogue and is not its reference."""
import numpy as np

METRICS = ('jaccard', 'hamming', 'dice', 'rogerstanimoto', 'russellrao', 'sokalmichener', 'sokalsneath', 'yule')


def distance_from_counts(metric, ntt, ntf, nft, n):
    ntt, ntf, nft, n = (np.asarray(v, dtype=np.float64) for v in (ntt, ntf, nft, n))
    nff = n - ntt - ntf - nft
    ndiff = ntf + nft
    with np.errstate(invalid='ignore', divide='ignore'):
        if metric == 'jaccard':
            den = ntt + ndiff
            return np.where(den == 0, 0.0, ndiff / np.where(den == 0, 1.0, den))
        if metric == 'hamming':
            return ndiff / n
        if metric == 'dice':
            return ndiff / (2.0 * ntt + ndiff)
        if metric in ('rogerstanimoto', 'sokalmichener'):
            return (2.0 * ndiff) / (n + ndiff)
        if metric == 'russellrao':
            return (n - ntt) / n
        if metric == 'sokalsneath':
            return (2.0 * ndiff) / (2.0 * ndiff + ntt)
        if metric == 'yule':
            half_r = ntf * nft
            return np.where(half_r == 0, 0.0, (2.0 * half_r) / np.where(half_r == 0, 1.0, ntt * nff + half_r))
    raise ValueError(metric)


def profiles_from_counts(ntt, ntf, nft, nff):
    """Two f64 0/1 profiles [2, n] with the given contingency counts."""
    x = np.concatenate([np.ones(ntt), np.ones(ntf), np.zeros(nft), np.zeros(nff)])
    y = np.concatenate([np.ones(ntt), np.zeros(ntf), np.ones(nft), np.zeros(nff)])
    return np.stack([x, y])
