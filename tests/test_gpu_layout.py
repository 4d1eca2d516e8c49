"""Edge-list networks through the device spring-embedded layout (safe_layout_spring, layout.hip), held to bit
equality with the real reference (tests/golden/layout.npz, made by tests/golden/make_layout_golden.py from
safe_io.load_network_from_txt / apply_network_layout, networkx 3.4.2):

  - coordinates of every case: networkx's f64 form below 500 nodes, its f32 form from 500 (the 499 / 500
    boundary, ~4000 nodes), 1 and 2 nodes, .txt / .tsv / .gz, weighted graphs with a self-loop
  - SAFE().load_network(network_file=...) -> x, y, length, the nodes frame, and define_neighborhoods()'s
    default-metric membership
  - the loaded graph as a whole input: compute_pvalues against the oracle on the reference's membership
  - seed=None draws from NumPy's global stream exactly as the reference does
  - a live cross-check against the installed networkx"""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    import safepy_amd
    assert safepy_amd.device_count() >= 1
    return dict(np.load(os.path.join(HERE, 'golden', 'layout.npz')))


def digest(a):
    """As tests/golden/make_layout_golden.py: sha256 of an array's C-order bytes."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def file_tags(g):
    return [t for t in g['tags'].tolist() if t + '_file' in g]


def write_case(g, tag, tmp_path):
    path = tmp_path / str(g[tag + '_name'])
    path.write_bytes(g[tag + '_file'].tobytes())
    return str(path)


def seed_of(g, tag):
    s = int(g[tag + '_seed'])
    return None if s < 0 else s


def coords(G):
    n = G.number_of_nodes()
    return (np.array([G.nodes[i]['x'] for i in range(n)], dtype=np.float64),
            np.array([G.nodes[i]['y'] for i in range(n)], dtype=np.float64))


def edge_lengths(G):
    e = sorted((min(u, v), max(u, v), d.get('length', np.nan)) for u, v, d in G.edges(data=True))
    return (np.array([x[:2] for x in e], dtype=np.int64).reshape(-1, 2), np.array([x[2] for x in e], dtype=np.float64))


def assert_graph_equals(g, tag, G):
    x, y = coords(G)
    assert np.array_equal(x, g[tag + '_x']), '%s: x differs at %d nodes' % (tag, int((x != g[tag + '_x']).sum()))
    assert np.array_equal(y, g[tag + '_y']), '%s: y differs at %d nodes' % (tag, int((y != g[tag + '_y']).sum()))
    edges, length = edge_lengths(G)
    if tag + '_edges' in g:                            # arrays up to 300 nodes, digests for every case
        assert np.array_equal(edges, g[tag + '_edges']), tag
        assert np.array_equal(length, g[tag + '_length'], equal_nan=True), tag
    assert digest(edges) == str(g[tag + '_edges_sha']), tag
    assert digest(length) == str(g[tag + '_length_sha']), '%s: edge lengths differ' % tag


def test_load_network_from_txt_coordinates_bit_equal(golden, tmp_path):
    from safepy_amd import safe_io
    for tag in file_tags(golden):
        state = np.random.get_state()
        np.random.seed(123)                            # the seed=None case draws from the global stream
        G = safe_io.load_network_from_txt(write_case(golden, tag, tmp_path), seed=seed_of(golden, tag), verbose=False)
        np.random.set_state(state)
        assert_graph_equals(golden, tag, G)


def test_apply_network_layout_weighted_self_loop_bit_equal(golden):
    import networkx as nx
    from safepy_amd import safe_io
    for tag in ('w60', 'w520'):
        G = nx.Graph()
        G.add_nodes_from(range(golden[tag + '_x'].size))
        for (u, v), w in zip(golden[tag + '_edges_in'].tolist(), golden[tag + '_weight_in'].tolist()):
            G.add_edge(u, v, weight=w)
        safe_io.apply_network_layout(G, layout='spring_embedded', seed=int(golden[tag + '_seed']), verbose=False)
        x, y = coords(G)
        assert np.array_equal(x, golden[tag + '_x']) and np.array_equal(y, golden[tag + '_y']), tag


def test_safe_load_network_and_default_neighborhoods(golden, tmp_path):
    import pandas as pd
    import safepy_amd
    for tag in [t for t in file_tags(golden) if t + '_membership' in golden]:
        sf = safepy_amd.SAFE(verbose=False)
        sf.random_seed = seed_of(golden, tag)
        sf.load_network(network_file=write_case(golden, tag, tmp_path))
        assert_graph_equals(golden, tag, sf.graph)
        n = golden[tag + '_x'].size
        want = pd.DataFrame({'id': list(range(n)), 'key': golden[tag + '_key'].tolist(),
                             'label': golden[tag + '_label'].tolist()})
        got = sf.nodes.copy()
        got['key'] = got['key'].astype(str)
        got['label'] = got['label'].astype(str)
        pd.testing.assert_frame_equal(got.reset_index(drop=True), want, check_dtype=False)
        sf.define_neighborhoods()
        member = np.packbits(np.asarray(sf.neighborhoods, dtype=bool), axis=1)
        assert np.array_equal(member, golden[tag + '_membership']), tag


def test_loaded_network_feeds_compute_pvalues(golden, tmp_path):
    """load_network(.tsv) -> load_attributes -> compute_pvalues, seeded, against the oracle run on the
    reference's own membership of the same file."""
    import safepy_amd
    from oracle import safe_oracle as orc
    tag = 'tsv700'
    n = golden[tag + '_x'].size
    sf = safepy_amd.SAFE(verbose=False)
    sf.random_seed = seed_of(golden, tag)
    sf.load_network(network_file=write_case(golden, tag, tmp_path))
    sf.define_neighborhoods()
    rng = np.random.default_rng(5)
    b = (rng.uniform(size=(n, 12)) < 0.1).astype(np.float64)
    b[rng.choice(n, 40, replace=False)] = np.nan
    sf.load_attributes(attribute_file=b.copy())
    sf.compute_pvalues(how='randomization', num_permutations=200, verbose=False)
    a = np.unpackbits(golden[tag + '_membership'], axis=1, count=n).astype(np.int64)
    want = orc.compute_pvalues(a, b.copy(), enrichment_type='randomization', num_permutations=200,
                               random_seed=sf.random_seed)
    for key in ('ns', 'pvalues_neg', 'pvalues_pos', 'nes', 'nes_binary'):
        assert np.array_equal(getattr(sf, key), want[key]), key


def test_seed_none_advances_the_global_stream_like_the_reference(golden, tmp_path):
    from safepy_amd import safe_io
    tag = 'seednone'
    assert seed_of(golden, tag) is None
    np.random.seed(123)
    G = safe_io.load_network_from_txt(write_case(golden, tag, tmp_path), seed=None, verbose=False)
    assert np.random.rand() == float(golden[tag + '_next_rand'])
    x, y = coords(G)
    assert np.array_equal(x, golden[tag + '_x']) and np.array_equal(y, golden[tag + '_y'])


def test_layout_graph_and_iterations_run(golden):
    """A LayoutGraph takes the same path (its .xy is set); the device reports how many iterations ran."""
    import safepy_amd
    from safepy_amd import backend as be, safe_io
    tag = 'w60'
    eu, ev = golden[tag + '_edges_in'].T
    lg = safepy_amd.LayoutGraph(np.zeros((golden[tag + '_x'].size, 2)), eu, ev, weight=golden[tag + '_weight_in'])
    safe_io.apply_network_layout(lg, layout='spring_embedded', seed=int(golden[tag + '_seed']), verbose=False)
    assert np.array_equal(lg.xy[:, 0], golden[tag + '_x']) and np.array_equal(lg.xy[:, 1], golden[tag + '_y'])
    # iterations: 0 leaves the initial draw; a huge threshold stops after the first
    ctx = be.Context.default(0)
    pos0 = np.random.RandomState(0).rand(600, 2)
    rp = np.zeros(601, np.int32)
    pos, ran = ctx.layout_spring(rp, np.zeros(0, np.int32), None, pos0, 0.2, 0, 1e-4, np.float32)
    assert ran == 0 and np.array_equal(pos, pos0.astype(np.float32))
    _, ran = ctx.layout_spring(rp, np.zeros(0, np.int32), None, pos0, 0.2, 100, 1e9, np.float32)
    assert ran == 1


def test_live_networkx_cross_check():
    """apply_network_layout against the installed networkx, rescale and f32 weight rounding included: two random geometric
    graphs (120 and 600 nodes), a dense graph (140 nodes, half of all pairs: more neighbour entries per 16 x 128 block
    than one round of the kernel's scatter) and one whose size is a whole number of 128-column chunks (512 nodes, f32
    form), the last two with weights that are not f32 numbers.  networkx's f32 form takes 80 - 190 us per row per iteration
    on the host: N = 600 costs this test 5 - 12 s of networkx time and N = 512 another 4 - 10 s."""
    nx = pytest.importorskip('networkx')
    from safepy_amd import safe_io
    graphs = []
    for n, seed in ((120, 3), (600, 4)):
        G = nx.random_geometric_graph(n, 0.12, seed=seed)
        for u, v in list(G.edges())[::3]:
            G[u][v]['weight'] = 0.5 + (u % 7) / 4
        graphs.append((n, seed, G))
    for n, p, seed in ((140, 0.5, 5), (512, 0.05, 6)):
        G = nx.gnp_random_graph(n, p, seed=seed)
        for u, v in list(G.edges())[::3]:
            G[u][v]['weight'] = 0.1 * (1 + (u + v) % 9)
        assert any(float(np.float32(d['weight'])) != d['weight'] for _, _, d in G.edges(data=True) if 'weight' in d)
        graphs.append((n, seed, G))
    for n, seed, G in graphs:
        want = nx.spring_layout(G, k=0.2, iterations=100, seed=seed)
        H = G.copy()
        safe_io.apply_network_layout(H, layout='spring_embedded', seed=seed, verbose=False)
        got = np.array([[H.nodes[i]['x'], H.nodes[i]['y']] for i in range(n)])
        assert np.array_equal(got, np.array([want[i] for i in range(n)])), n
