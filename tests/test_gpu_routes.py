"""Which kernel family each enrichment entry point runs (enrich.hip: perm_route for the permutation test, counts_route for
the binary 'sum' counts) for every value of the routing switches.  The expected names are the ones the library gave before
the routes were gathered into those two functions; the permutation-test cases also check that safe_randomization_plan
predicts the bit-sliced layout exactly when the bit-sliced kernel runs.  Small inputs: the file runs in seconds.
Needs an MI355X."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import safe_oracle as orc            # noqa: E402  (radius rule only)

# every switch that steers a route; each case sets the ones it names and clears the others
SWITCHES = {'F': 'SAFE_HIP_FORCE_PATH', 'NARROW': 'SAFE_HIP_NARROW_LDS', 'COUNTS': 'SAFE_HIP_COUNTS',
            'TABLE': 'SAFE_HIP_HYPER_TABLE', 'MFMA_Z': 'SAFE_HIP_MFMA_Z', 'SPLIT': 'SAFE_HIP_HYP_SPLIT'}
NPERM, SEED = 20, 7

# data kind -> (nodes, columns, values, membership)
#   bin       sparse euclidean membership, 0/1 columns (some all-NaN rows)
#   bin_hub   one neighborhood holds every node (2100 >= 2048 members: no bit-sliced form)
#   dense     a random membership of ~60 % density (nnz >= 128 n: the matrix cores' counts rule)
#   q_small   quantitative, N = 200 (below one 256-row group)
#   q_narrow  quantitative, N x columns <= 204 800 (a narrow block)
#   q_wide    quantitative, N x columns > 204 800
#   q_decline 1e18 next to 1e-3 in one column: the matrix cores decline it (test_gpu_mfma.py)
#   q_big_n   N = 5200: the LDS-resident f64 kernel does not fit
DATA = {'bin': (300, 16, 'bin', 'euclid'), 'bin_hub': (2100, 8, 'bin', 'hub'), 'dense': (300, 16, 'bin', 'dense'),
        'q_small': (200, 4, 'quant', 'euclid'), 'q_narrow': (600, 8, 'quant', 'euclid'), 'q_wide': (1000, 256, 'quant', 'euclid'),
        'q_decline': (300, 8, 'decline', 'euclid'), 'q_big_n': (5200, 2, 'quant', 'euclid')}

PERM_CASES = [
    ('bin', 'sum', {}), ('bin', 'sum', {'F': 'bits'}), ('bin', 'sum', {'F': 'scatter'}), ('bin', 'sum', {'F': 'gather'}),
    ('bin', 'sum', {'F': 'lds'}), ('bin', 'sum', {'F': 'mfma'}), ('bin', 'sum', {'NARROW': '0'}), ('bin', 'z-score', {}),
    ('bin_hub', 'sum', {}), ('bin_hub', 'sum', {'F': 'bits'}), ('bin_hub', 'sum', {'F': 'scatter'}),
    ('dense', 'sum', {}), ('dense', 'sum', {'COUNTS': 'mfma', 'TABLE': '0'}),
    ('q_small', 'sum', {}), ('q_small', 'sum', {'F': 'mfma'}),
    ('q_narrow', 'sum', {}), ('q_narrow', 'sum', {'NARROW': '0'}), ('q_narrow', 'sum', {'F': 'mfma'}),
    ('q_narrow', 'sum', {'F': 'lds'}), ('q_narrow', 'sum', {'F': 'gather'}), ('q_narrow', 'sum', {'F': 'bits'}),
    ('q_narrow', 'sum', {'F': 'scatter'}), ('q_narrow', 'z-score', {}), ('q_narrow', 'z-score', {'NARROW': '0'}),
    ('q_narrow', 'z-score', {'NARROW': '0', 'MFMA_Z': '0'}),
    ('q_wide', 'sum', {}), ('q_wide', 'sum', {'F': 'lds'}), ('q_wide', 'z-score', {}), ('q_wide', 'z-score', {'MFMA_Z': '0'}),
    ('q_decline', 'sum', {}), ('q_decline', 'sum', {'NARROW': '0'}), ('q_decline', 'sum', {'NARROW': '0', 'F': 'mfma'}),
    ('q_big_n', 'sum', {}), ('q_big_n', 'z-score', {'MFMA_Z': '0'}), ('q_big_n', 'sum', {'F': 'lds'}),
]
COUNT_CASES = [
    ('bin', 'sum', {}), ('bin', 'sum', {'COUNTS': 'mfma'}), ('bin', 'sum', {'COUNTS': 'bits'}), ('bin', 'sum', {'F': 'gather'}),
    ('bin', 'sum', {'F': 'lds'}), ('bin', 'sum', {'TABLE': '0'}), ('bin', 'sum', {'TABLE': '0', 'COUNTS': 'mfma'}),
    ('bin', 'sum', {'COUNTS': 'mfma', 'SPLIT': '0'}), ('bin', 'z-score', {}),
    ('dense', 'sum', {}), ('dense', 'sum', {'SPLIT': '0'}), ('dense', 'sum', {'COUNTS': 'bits'}),
    ('dense', 'sum', {'TABLE': '0'}), ('dense', 'sum', {'F': 'mfma'}), ('dense', 'sum', {'F': 'gather'}),
    ('bin_hub', 'sum', {}), ('bin_hub', 'sum', {'COUNTS': 'mfma'}),
    ('q_narrow', 'sum', {}), ('q_narrow', 'z-score', {}),
]


def _case_id(entry, kind, score, env):
    return '-'.join([entry, kind, score] + ['%s=%s' % kv for kv in sorted(env.items())])


CASES = ([(e, *c) for e in ('permtest_counts', 'randomization') for c in PERM_CASES] +
         [(e, *c) for e in ('score', 'hypergeom') for c in COUNT_CASES if not (e == 'hypergeom' and c[1] != 'sum')])


def make_data(be, ctx, kind):
    """(membership handle, attribute handle, n, m) of a data kind, the same on every run."""
    n, m, values, memb = DATA[kind]
    rng = np.random.default_rng(n + m)
    xy = rng.uniform(size=(n, 2))
    if memb == 'euclid':
        nbr = be.Neighborhoods.euclidean(ctx, xy, orc.layout_radius(xy[:, 0], float(np.sqrt(10.0 / (np.pi * n)))))
    else:
        a = (rng.uniform(size=(n, n)) < (0.6 if memb == 'dense' else 0.004)).astype(np.int64)
        if memb == 'hub':
            a[5, :] = 1
        nbr = be.Neighborhoods.from_dense(ctx, a)
    if values == 'bin':
        b = (rng.uniform(size=(n, m)) < 0.1).astype(np.float64)
        b[rng.choice(n, n // 30, replace=False)] = np.nan
    else:
        b = rng.normal(size=(n, m)) * (1e-3 if values == 'decline' else 1.0)
        if values == 'decline':
            b[7, 2] = 1e18
    return nbr, be.Attributes.from_host(ctx, b), n, m


def run_case(be, ctx, data, entry, kind, score, env, setenv, delenv):
    """Runs one case with the switches of `env` set (and the others cleared) through setenv / delenv; returns (last kernel
    name, randomization_plan or None, SHA-256 of every output)."""
    for key, var in SWITCHES.items():
        if key in env:
            setenv(var, env[key])
        else:
            delenv(var)
    nbr, attr, n, m = data[kind]
    shapes = {'permtest_counts': [(n, m)] * 3, 'randomization': [(n, m)] * 5 + [(m,)], 'score': [(n, m)],
              'hypergeom': [(n, m)] * 3 + [(m,)]}[entry]
    bufs = [ctx.alloc_f64(*shape) for shape in shapes]
    for b in bufs:
        b.zero()
    ptrs = [b.ptr for b in bufs]
    plan = None
    if entry in ('permtest_counts', 'randomization'):
        plan = be.randomization_plan(ctx, nbr, attr, NPERM, score)
        perms = be.Permutations(ctx, n, attr.row_flags(), NPERM, SEED)
        if entry == 'permtest_counts':
            be.permtest_counts(ctx, nbr, attr, perms, score, *ptrs)
        else:
            be.randomization(ctx, nbr, attr, perms, score, 'both', 0.05, ptrs)
        name = ctx.last_kernel()[0]
        perms.close()
    else:
        if entry == 'score':
            be.score(ctx, nbr, attr, score, ptrs[0])
        else:
            be.hypergeom(ctx, nbr, attr, 0.05, ptrs)
        name = ctx.last_kernel()[0]
    digest = hashlib.sha256()
    for b, shape in zip(bufs, shapes):
        digest.update(b.download(shape).tobytes())
    return name, plan, digest.hexdigest()


# recorded on the parent of the change that introduced perm_route / counts_route.  Routes by name: k_permtest_bits_* BITS,
# k_permtest_scatter SCATTER, k_permtest_mfma MFMA, k_permtest_lds LDS_F64 (q_decline and q_wide: after the matrix cores
# declined), k_permtest_gather* GATHER; counts: k_counts_bits* bit-sliced, k_permtest_mfma<counts> / k_hyp_emit on the
# matrix cores, k_permtest_gather* / k_hypergeom_tail not bit-sliced (or the per-element hypergeometric kernel)
EXPECTED = {
    'permtest_counts-bin-sum': 'k_permtest_bits_blk',
    'permtest_counts-bin-sum-F=bits': 'k_permtest_bits_blk',
    'permtest_counts-bin-sum-F=scatter': 'k_permtest_scatter',
    'permtest_counts-bin-sum-F=gather': 'k_permtest_gather<16,false>',
    'permtest_counts-bin-sum-F=lds': 'k_permtest_bits_blk',
    'permtest_counts-bin-sum-F=mfma': 'k_permtest_bits_blk',
    'permtest_counts-bin-sum-NARROW=0': 'k_permtest_bits_blk',
    'permtest_counts-bin-z-score': 'k_permtest_lds',
    'permtest_counts-bin_hub-sum': 'k_permtest_scatter',
    'permtest_counts-bin_hub-sum-F=bits': 'k_permtest_scatter',
    'permtest_counts-bin_hub-sum-F=scatter': 'k_permtest_scatter',
    'permtest_counts-dense-sum': 'k_permtest_bits_blk',
    'permtest_counts-dense-sum-COUNTS=mfma-TABLE=0': 'k_permtest_bits_blk',
    'permtest_counts-q_small-sum': 'k_permtest_lds',
    'permtest_counts-q_small-sum-F=mfma': 'k_permtest_mfma',
    'permtest_counts-q_narrow-sum': 'k_permtest_lds',
    'permtest_counts-q_narrow-sum-NARROW=0': 'k_permtest_mfma',
    'permtest_counts-q_narrow-sum-F=mfma': 'k_permtest_mfma',
    'permtest_counts-q_narrow-sum-F=lds': 'k_permtest_lds',
    'permtest_counts-q_narrow-sum-F=gather': 'k_permtest_gather<16,false>',
    'permtest_counts-q_narrow-sum-F=bits': 'k_permtest_lds',
    'permtest_counts-q_narrow-sum-F=scatter': 'k_permtest_lds',
    'permtest_counts-q_narrow-z-score': 'k_permtest_lds',
    'permtest_counts-q_narrow-z-score-NARROW=0': 'k_permtest_mfma',
    'permtest_counts-q_narrow-z-score-MFMA_Z=0-NARROW=0': 'k_permtest_lds',
    'permtest_counts-q_wide-sum': 'k_permtest_lds',
    'permtest_counts-q_wide-sum-F=lds': 'k_permtest_lds',
    'permtest_counts-q_wide-z-score': 'k_permtest_lds',
    'permtest_counts-q_wide-z-score-MFMA_Z=0': 'k_permtest_lds',
    'permtest_counts-q_decline-sum': 'k_permtest_lds',
    'permtest_counts-q_decline-sum-NARROW=0': 'k_permtest_lds',
    'permtest_counts-q_decline-sum-F=mfma-NARROW=0': 'k_permtest_mfma',
    'permtest_counts-q_big_n-sum': 'k_permtest_mfma',
    'permtest_counts-q_big_n-z-score-MFMA_Z=0': 'k_permtest_gather<8,true>',
    'permtest_counts-q_big_n-sum-F=lds': 'k_permtest_gather<16,false>',
    'randomization-bin-sum': 'k_permtest_bits_blk',
    'randomization-bin-sum-F=bits': 'k_permtest_bits_blk',
    'randomization-bin-sum-F=scatter': 'k_permtest_scatter',
    'randomization-bin-sum-F=gather': 'k_permtest_gather<16,false>',
    'randomization-bin-sum-F=lds': 'k_permtest_bits_blk',
    'randomization-bin-sum-F=mfma': 'k_permtest_bits_blk',
    'randomization-bin-sum-NARROW=0': 'k_permtest_bits_blk',
    'randomization-bin-z-score': 'k_permtest_lds',
    'randomization-bin_hub-sum': 'k_permtest_scatter',
    'randomization-bin_hub-sum-F=bits': 'k_permtest_scatter',
    'randomization-bin_hub-sum-F=scatter': 'k_permtest_scatter',
    'randomization-dense-sum': 'k_permtest_bits_blk',
    'randomization-dense-sum-COUNTS=mfma-TABLE=0': 'k_permtest_bits_blk',
    'randomization-q_small-sum': 'k_permtest_lds',
    'randomization-q_small-sum-F=mfma': 'k_permtest_mfma',
    'randomization-q_narrow-sum': 'k_permtest_lds',
    'randomization-q_narrow-sum-NARROW=0': 'k_permtest_mfma',
    'randomization-q_narrow-sum-F=mfma': 'k_permtest_mfma',
    'randomization-q_narrow-sum-F=lds': 'k_permtest_lds',
    'randomization-q_narrow-sum-F=gather': 'k_permtest_gather<16,false>',
    'randomization-q_narrow-sum-F=bits': 'k_permtest_lds',
    'randomization-q_narrow-sum-F=scatter': 'k_permtest_lds',
    'randomization-q_narrow-z-score': 'k_permtest_lds',
    'randomization-q_narrow-z-score-NARROW=0': 'k_permtest_mfma',
    'randomization-q_narrow-z-score-MFMA_Z=0-NARROW=0': 'k_permtest_lds',
    'randomization-q_wide-sum': 'k_permtest_lds',
    'randomization-q_wide-sum-F=lds': 'k_permtest_lds',
    'randomization-q_wide-z-score': 'k_permtest_lds',
    'randomization-q_wide-z-score-MFMA_Z=0': 'k_permtest_lds',
    'randomization-q_decline-sum': 'k_permtest_lds',
    'randomization-q_decline-sum-NARROW=0': 'k_permtest_lds',
    'randomization-q_decline-sum-F=mfma-NARROW=0': 'k_permtest_mfma',
    'randomization-q_big_n-sum': 'k_permtest_mfma',
    'randomization-q_big_n-z-score-MFMA_Z=0': 'k_permtest_gather<8,true>',
    'randomization-q_big_n-sum-F=lds': 'k_permtest_gather<16,false>',
    'score-bin-sum': 'k_counts_bits',
    'score-bin-sum-COUNTS=mfma': 'k_permtest_mfma<counts>',
    'score-bin-sum-COUNTS=bits': 'k_counts_bits',
    'score-bin-sum-F=gather': 'k_permtest_gather<16,false>',
    'score-bin-sum-F=lds': 'k_counts_bits',
    'score-bin-sum-TABLE=0': 'k_counts_bits',
    'score-bin-sum-COUNTS=mfma-TABLE=0': 'k_permtest_mfma<counts>',
    'score-bin-sum-COUNTS=mfma-SPLIT=0': 'k_permtest_mfma<counts>',
    'score-bin-z-score': 'k_permtest_gather<8,true>',
    'score-dense-sum': 'k_permtest_mfma<counts>',
    'score-dense-sum-SPLIT=0': 'k_permtest_mfma<counts>',
    'score-dense-sum-COUNTS=bits': 'k_counts_bits',
    'score-dense-sum-TABLE=0': 'k_permtest_mfma<counts>',
    'score-dense-sum-F=mfma': 'k_permtest_mfma<counts>',
    'score-dense-sum-F=gather': 'k_permtest_gather<16,false>',
    'score-bin_hub-sum': 'k_permtest_gather<16,false>',
    'score-bin_hub-sum-COUNTS=mfma': 'k_permtest_gather<16,false>',
    'score-q_narrow-sum': 'k_permtest_gather<16,false>',
    'score-q_narrow-z-score': 'k_permtest_gather<8,true>',
    'hypergeom-bin-sum': 'k_counts_bits<hypergeom>',
    'hypergeom-bin-sum-COUNTS=mfma': 'k_hyp_emit',
    'hypergeom-bin-sum-COUNTS=bits': 'k_counts_bits<hypergeom>',
    'hypergeom-bin-sum-F=gather': 'k_hypergeom_tail',
    'hypergeom-bin-sum-F=lds': 'k_counts_bits<hypergeom>',
    'hypergeom-bin-sum-TABLE=0': 'k_hypergeom_tail',
    'hypergeom-bin-sum-COUNTS=mfma-TABLE=0': 'k_hypergeom_tail',
    'hypergeom-bin-sum-COUNTS=mfma-SPLIT=0': 'k_permtest_mfma<counts>',
    'hypergeom-dense-sum': 'k_hyp_emit',
    'hypergeom-dense-sum-SPLIT=0': 'k_permtest_mfma<counts>',
    'hypergeom-dense-sum-COUNTS=bits': 'k_counts_bits<hypergeom>',
    'hypergeom-dense-sum-TABLE=0': 'k_hypergeom_tail',
    'hypergeom-dense-sum-F=mfma': 'k_hyp_emit',
    'hypergeom-dense-sum-F=gather': 'k_hypergeom_tail',
    'hypergeom-bin_hub-sum': 'k_hypergeom_tail',
    'hypergeom-bin_hub-sum-COUNTS=mfma': 'k_hypergeom_tail',
    'hypergeom-q_narrow-sum': 'k_hypergeom_tail',
}


@pytest.fixture(scope='module')
def setup():
    import safepy_amd
    from safepy_amd import backend as be
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    ctx = be.Context.default(0)
    data = {k: make_data(be, ctx, k) for k in DATA}
    yield be, ctx, data
    for nbr, attr, _, _ in data.values():
        attr.close()
        nbr.close()


@pytest.mark.parametrize('case', CASES, ids=[_case_id(*c) for c in CASES])
def test_route(setup, monkeypatch, case):
    be, ctx, data = setup
    name, plan, _ = run_case(be, ctx, data, *case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    assert name == EXPECTED[_case_id(*case)]
    if plan is not None:
        assert (plan == 0) == name.startswith('k_permtest_bits')
