"""SAFE.print_output_files / SAFE.save (safepy/safe.py:1267-1306, 237-242) and the device formatter behind the node table
(safe_format_tsv, safepy_amd/csrc/format.hip): byte equality with NumPy's text of every value, with pandas' to_csv of the
same tables, and with the real reference's files (tests/golden/output_files.npz, make_output_golden.py).  Needs an MI355X."""
import os
import pickle
import re

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'output_files.npz')


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


def texts(x):
    """What pandas writes for each value of a float block: repr(float) (= NumPy's astype(str)), NaN empty."""
    return ['' if s == 'nan' else s for s in map(repr, x.ravel().tolist())]


def expected_rows(x, prefixes):
    n, m = x.shape
    t = texts(x)
    return b''.join(prefixes[i] + ''.join('\t' + s for s in t[i * m:(i + 1) * m]).encode() + b'\n' for i in range(n))


def device_format(amd, tmp_path, x, prefixes, budget=None, r0=0, r1=None):
    from safepy_amd import backend as be
    ctx = be.Context.default(0)
    n, m = x.shape
    r1 = n if r1 is None else r1
    buf = ctx.alloc_f64(n, max(m, 1))
    try:
        if x.size:
            buf.upload(np.ascontiguousarray(x))
        off = np.zeros(r1 - r0 + 1, dtype=np.int64)
        np.cumsum([len(p) for p in prefixes[r0:r1]], out=off[1:])
        path = str(tmp_path / 'fmt.txt')
        with open(path, 'wb') as f:
            stats = ctx.format_tsv(buf.ptr, n, m, b''.join(prefixes[r0:r1]), off, f.fileno(), r0=r0, r1=r1, budget_bytes=budget)
        data = open(path, 'rb').read()
        assert stats['bytes'] == len(data)
        return data
    finally:
        buf.free()


def curated():
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308,
         9.999999999999999e-05, 1e-4, 9999999999999998.0, 1e16]
    v += [float('1e%d' % k) for k in range(-323, 309)]
    v += [2.0 ** k for k in range(-1074, 1024)]
    v += [float(2 ** 53 + d) for d in range(-8, 9)]
    for p in (100, 1000, 10000):
        v += list(-np.log10(np.arange(1, p + 1) / p))
    bits = np.array(v, dtype=np.float64).view(np.uint64)
    with np.errstate(over='ignore'):
        bits = np.concatenate([bits, bits + np.uint64(1), bits - np.uint64(1)])
    x = bits.view(np.float64)
    return np.concatenate([x, -x])


def test_random_bit_patterns_against_numpy(amd, tmp_path):
    """2 * 10^7 uniformly random 64-bit patterns (every exponent, NaN payloads, subnormals) in rows of 4373 values."""
    rng = np.random.default_rng(11)
    m = 4373
    for part in range(5):
        x = rng.integers(0, 2 ** 64, size=(915, m), dtype=np.uint64, endpoint=False).view(np.float64)
        prefixes = [b'%d' % (part * 915 + i) for i in range(x.shape[0])]
        got = device_format(amd, tmp_path, x, prefixes)
        want = expected_rows(x, prefixes)
        assert got == want, 'part %d: first difference at byte %d' % (part, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
                                                                      if len(got) == len(want) else min(len(got), len(want)))
    sub = x[:2].ravel()
    assert ['' if s == 'nan' else s for s in sub.astype(str).tolist()] == texts(sub)


@pytest.mark.parametrize('m', [1, 7, 4373])
def test_curated_values_every_shape(amd, tmp_path, m):
    """The curated set laid out as [N, M] with N not a multiple of anything the kernels use, prefixes of every length
    (empty, one byte, longer than the kernel's 4096-byte prefix piece), against NumPy's astype(str)."""
    x = curated()
    rng = np.random.default_rng(m)
    x = x[rng.permutation(x.size)]
    n = -(-x.size // m)
    n += 1 if n % 2 == 0 else 0
    x = np.resize(x, n * m).reshape(n, m)
    prefixes = [b'' if i % 5 == 0 else (b'r%d\t"k ""%d"""' % (i, i) if i % 7 else b'x' * (5000 + i)) for i in range(n)]
    want_text = x.astype(str)
    want_text[np.isnan(x)] = ''
    want = b''.join(prefixes[i] + ''.join('\t' + s for s in want_text[i]).encode() + b'\n' for i in range(n))
    assert device_format(amd, tmp_path, x, prefixes) == want


def test_small_budget_runs_many_chunks(amd, tmp_path):
    """Chunks of one row (a budget below one row's bound) and of a few rows: the two pinned buffers alternate and the
    rows written are exactly those of [r0, r1)."""
    rng = np.random.default_rng(3)
    x = -np.log10(rng.integers(1, 1001, size=(301, 333)) / 1000.0)
    x[rng.uniform(size=x.shape) < 0.05] = np.nan
    x[5] = np.nan
    prefixes = [b'%d\tK%d\tL%d' % (i, i, i) for i in range(301)]
    want = expected_rows(x, prefixes)
    for budget in (1, 40_000, 1 << 30):
        assert device_format(amd, tmp_path, x, prefixes, budget=budget) == want, budget
    part = device_format(amd, tmp_path, x, prefixes, budget=50_000, r0=17, r1=290)
    assert part == expected_rows(x[17:290], prefixes[17:290])
    assert device_format(amd, tmp_path, np.zeros((4, 0)), [b'a', b'', b'c', b'd']) == b'a\n\nc\nd\n'


# ------------------------------------------------------------------------------------ the whole call ----
def pandas_node_table(sf):
    """The reference's own code for the node table without domains (safe.py:1286-1306), from the object's host arrays."""
    import networkx as nx
    keys = list(nx.get_node_attributes(sf.graph, 'key').values())
    labels = list(nx.get_node_attributes(sf.graph, 'label').values())
    nodes = pd.DataFrame(sf.nes)
    nodes.columns = sf.attributes['name']
    nodes.insert(loc=0, column='key', value=keys)
    nodes.insert(loc=1, column='label', value=labels)
    return nodes


@pytest.fixture(scope='module')
def example3(tmp_path_factory):
    from safepy_amd import workloads
    path = str(tmp_path_factory.mktemp('ex3') / 'surrogate_UMAP_1586.scatter')
    return path, workloads.example3_scatter(path)


def example3_safe(amd, example3, how, lazy):
    path, (keys, xy, att) = example3
    sf = amd.SAFE(verbose=False)
    sf.lazy_outputs = lazy
    sf.random_seed = 7
    sf.load_network(network_file=path, node_key_attribute='key')
    if how == 'hypergeometric':
        # a binary attribute (the left half of the layout) and wide neighborhoods: p-values down to 1e-300 and below (where
        # one underflows to 0 its NES is inf; the text of +-inf itself is pinned by test_curated_values_every_shape)
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.5)
        att = pd.DataFrame({'left': (xy[:, 0] < np.median(xy[:, 0])).astype(np.float64)}, index=att.index)
    else:
        sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.06)
    sf.load_attributes(attribute_file=att)
    sf.compute_pvalues(how=how, num_permutations=1000)
    return sf


@pytest.mark.parametrize('how,lazy', [('randomization', True), ('randomization', False), ('hypergeometric', True)])
def test_example3_print_output_files_equals_pandas(amd, example3, tmp_path, how, lazy):
    """The reference's Example 3 ends with sf.print_output_files(output_dir='./'): the files equal pandas' to_csv of the
    same tables, built by the reference's code from the same host arrays -- with nes read in place on the device (the
    lazy default), with nes on the host (lazy_outputs = False), and for the hypergeometric test."""
    from safepy_amd.safe import _DeviceResult
    sf = example3_safe(amd, example3, how, lazy)
    assert isinstance(sf.__dict__['_r_nes'], _DeviceResult) == lazy
    sf.print_output_files(output_dir=str(tmp_path))
    assert sf.output_dir == str(tmp_path)
    assert not os.path.exists(tmp_path / 'domain_properties_annotation.txt')
    nodes = pandas_node_table(sf)
    if how == 'hypergeometric':
        assert np.nanmax(sf.nes) > 250 and not np.isnan(sf.nes).any()
    assert nodes.equals(sf.nodes)
    assert (tmp_path / 'node_properties_annotation.txt').read_bytes() == nodes.to_csv(sep='\t').encode()
    assert (tmp_path / 'attribute_properties_annotation.txt').read_bytes() == sf.attributes.to_csv(sep='\t').encode()
    t = sf.output_timing
    assert t['bytes'] > 0 and t['kernel_ms'] > 0


def test_wide_table_several_chunks_equals_pandas(amd, tmp_path):
    """A NES-form table of 600 x 700 with NaN rows and attribute names pandas quotes, formatted in chunks of ~100 rows."""
    rng = np.random.default_rng(5)
    n, m = 600, 700
    xy = rng.uniform(size=(n, 2))
    b = np.round(rng.standard_normal((n, m)) * 64) / 64
    b[rng.choice(n, 30, replace=False)] = np.nan
    keys = ['K%d' % i for i in range(n)]
    keys[3] = 'a "quoted" key'
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, keys=keys)
    sf.random_seed = 3
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.08)
    sf.load_attributes(attribute_file=b)
    sf.attributes['name'] = ['attr\t%d' % j if j % 50 == 0 else 'attr %d' % j for j in range(m)]
    sf.compute_pvalues(how='randomization', num_permutations=200)
    sf.print_output_files(output_dir=str(tmp_path), budget_bytes=100 * (25 * m + 40))
    nodes = pd.DataFrame(sf.nes)
    nodes.columns = sf.attributes['name']
    nodes.insert(loc=0, column='key', value=sf.graph.keys)
    nodes.insert(loc=1, column='label', value=sf.graph.labels)
    assert nodes.equals(sf.nodes)
    assert (tmp_path / 'node_properties_annotation.txt').read_bytes() == nodes.to_csv(sep='\t').encode()


def test_save_round_trip(amd, example3, tmp_path):
    sf = example3_safe(amd, example3, 'randomization', True)
    sf.save(output_file=str(tmp_path / 'sf.p'))
    with open(str(tmp_path / 'sf.p'), 'rb') as f:
        back = pickle.load(f)
    for key in ('nes', 'nes_binary', 'neighborhoods'):
        assert np.array_equal(getattr(back, key), getattr(sf, key), equal_nan=True), key
    assert back.attributes.equals(sf.attributes)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        sf.save()
    finally:
        os.chdir(cwd)
    assert (tmp_path / 'safe_output.p').exists()


# ------------------------------------------------------------------------------------ the reference ----
def replay(amd, g, tag):
    nperm, seed, domains = (int(v) for v in g[tag + 'meta'])
    xy, eu, ev = g[tag + 'xy'], g[tag + 'edge_u'], g[tag + 'edge_v']
    length = np.sqrt(((xy[eu] - xy[ev]) ** 2).sum(axis=1))
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(xy, eu, ev, length=length, keys=list(g[tag + 'keys']), labels=list(g[tag + 'labels']))
    sf.random_seed = seed
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.2)
    sf.load_attributes(attribute_file=g[tag + 'attributes'].copy())
    sf.attributes = pd.DataFrame({'id': np.arange(len(g[tag + 'names'])), 'name': list(g[tag + 'names'])})
    sf.compute_pvalues(how='randomization', num_permutations=nperm)
    if domains:
        sf.define_top_attributes()
        sf.define_domains()
        sf.trim_domains()
    return sf


@pytest.mark.parametrize('tag', ['nes_', 'dom_'])
def test_files_equal_the_reference(amd, tmp_path, tag):
    """Seeded randomization cases run through the real reference's print_output_files (make_output_golden.py): the same
    inputs through safepy_amd.SAFE give the same bytes in all three files."""
    g = dict(np.load(GOLDEN))
    sf = replay(amd, g, tag)
    sf.print_output_files(output_dir=str(tmp_path))
    for name in ('domain', 'attribute', 'node'):
        path = tmp_path / ('%s_properties_annotation.txt' % name)
        want = g[tag + name].tobytes()
        got = path.read_bytes() if path.exists() else b''
        if tag == 'dom_' and name == 'attribute':
            # size_connected_components of an attribute with ONE component: the reference's pandas .at assignment stores it
            # as a 0-d array (text "22"), define_top_attributes here as a one-element array ("[22]") -- a difference of
            # that method's object column, not of the writer; every other byte must match
            got = re.sub(rb'\t\[(\d+)\]\t', rb'\t\1\t', got)
        assert got == want, (name, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))
    if tag == 'dom_':
        assert 0 not in sf.domains.index and len(sf.domains) >= 2
        assert list(sf.nodes.columns) == ['id', 'key', 'label', 'domain', 'nes', 'num_domains']
        assert list(sf.nodes['key']) == list(g[tag + 'keys'])
        assert np.array_equal(sf.nodes['num_domains'].values, sf.node2domain[sf.domains['id']].sum(axis=1).values)
    else:
        assert list(sf.nodes.columns[:2]) == ['key', 'label'] and sf.nodes.shape == (len(g[tag + 'keys']), 2 + len(g[tag + 'names']))
