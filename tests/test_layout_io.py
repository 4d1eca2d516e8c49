"""Edge-list networks (.txt / .tsv, optionally .gz): the parse of load_network_from_txt (safepy/safe_io.py:30-107)
-- node numbering, labels, keys, edges -- against the reference's own graphs (tests/golden/layout.npz, made by
tests/golden/make_layout_golden.py), and the reference's errors for malformed files.  No GPU: the parse is
host code."""
import hashlib
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'layout.npz')))


def digest(a):
    """As tests/golden/make_layout_golden.py: sha256 of an array's C-order bytes or of newline-joined strings."""
    if isinstance(a, list):
        return hashlib.sha256('\n'.join(a).encode()).hexdigest()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def file_tags(g):
    return [t for t in g['tags'].tolist() if t + '_file' in g]


def write_case(g, tag, tmp_path):
    path = tmp_path / str(g[tag + '_name'])
    path.write_bytes(g[tag + '_file'].tobytes())
    return str(path)


def test_fixture_covers_the_cases(golden):
    tags = file_tags(golden)
    names = [str(golden[t + '_name']) for t in tags]
    assert any(n.endswith('.txt') for n in names) and any(n.endswith('.tsv') for n in names)
    assert any(n.endswith('.gz') for n in names)
    sizes = {golden[t + '_x'].size for t in tags}
    assert {499, 500}.issubset(sizes) and max(sizes) >= 4000
    # networkx's early stop (norm(delta_pos) / N < 1e-4) fired before iteration 100 in at least one case
    assert min(int(golden[t + '_iters']) for t in tags) < 100


def test_edge_list_parse_matches_reference(golden, tmp_path):
    from safepy_amd import safe_io
    for tag in file_tags(golden):
        data, nodes = safe_io._read_edge_list(write_case(golden, tag, tmp_path))
        labels, keys = nodes['node_label1'].astype(str).tolist(), nodes['node_key1'].astype(str).tolist()
        if tag + '_label' in golden:
            assert labels == golden[tag + '_label'].tolist() and keys == golden[tag + '_key'].tolist(), tag
        assert digest(labels) == str(golden[tag + '_label_sha']) and digest(keys) == str(golden[tag + '_key_sha']), tag
        u, v = data['node_index1'].to_numpy(), data['node_index2'].to_numpy()
        edges = np.unique(np.stack([np.minimum(u, v), np.maximum(u, v)], axis=1), axis=0).astype(np.int64)
        if tag + '_edges' in golden:
            assert np.array_equal(edges, golden[tag + '_edges']), tag
        assert digest(edges) == str(golden[tag + '_edges_sha']), tag


def test_one_and_two_node_files(tmp_path):
    from safepy_amd import safe_io
    p = tmp_path / 'one.txt'
    p.write_text('A\tA\t1.0\n')
    data, nodes = safe_io._read_edge_list(str(p))
    assert nodes['node_label1'].tolist() == ['A'] and data[['node_index1', 'node_index2']].values.tolist() == [[0, 0]]
    p = tmp_path / 'two.tsv'
    p.write_text('l1\tk1\tl2\tk2\tw\nb\tB\ta\tA\t2\n')
    data, nodes = safe_io._read_edge_list(str(p))
    assert nodes['node_label1'].tolist() == ['b', 'a'] and nodes['node_key1'].tolist() == ['B', 'A']
    assert data[['node_index1', 'node_index2']].values.tolist() == [[0, 1]]


@pytest.mark.parametrize('text', ['A\tB\n', 'A\tB\tC\t1.0\n', 'a\tA\tb\tB\t1\t9\n'])
def test_wrong_column_count_raises_value_error(tmp_path, text):
    from safepy_amd import safe_io
    p = tmp_path / 'bad.txt'
    p.write_text(text)
    with pytest.raises(ValueError, match='3 or 5 columns'):
        safe_io.load_network_from_txt(str(p), verbose=False)


def test_unsupported_extension_raises_value_error(tmp_path):
    from safepy_amd import safe_io
    p = tmp_path / 'net.csv'
    p.write_text('A\tB\t1\n')
    with pytest.raises(ValueError, match='not supported'):
        safe_io.load_network_from_txt(str(p), verbose=False)


def test_kamada_kawai_is_not_implemented():
    import networkx as nx
    from safepy_amd import safe_io
    with pytest.raises(NotImplementedError, match='spring_embedded'):
        safe_io.apply_network_layout(nx.path_graph(3), layout='kamada_kawai', seed=1, verbose=False)
