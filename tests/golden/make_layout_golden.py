#!/usr/bin/env python3
"""Golden vectors for edge-list networks and the spring-embedded layout, made by the REAL reference.

Run where the reference checkout exists (see make_golden.py's import_reference):

    python tests/golden/make_layout_golden.py

Writes tests/golden/layout.npz.  Edge-list files (.txt / .tsv, optionally gzipped) are generated from
seeded random geometric graphs, stored as raw bytes, and pushed through the reference's
``SAFE.load_network`` -> ``safe_io.load_network_from_txt`` (nx.spring_layout(k=0.2, iterations=100),
safe_io.py:288-308, then calculate_edge_lengths), and for some cases ``define_neighborhoods()`` with the
default settings.  A weighted in-memory graph with a self-loop goes through
``safe_io.apply_network_layout(G, 'spring_embedded', seed=...)``.  Per case <tag>:

    <tag>_file        the file's bytes (edge-list cases)          <tag>_name  its file name
    <tag>_seed        SAFE.random_seed / apply_network_layout's seed (-1 = None)
    <tag>_x, <tag>_y  node coordinates in node order              <tag>_iters iterations networkx ran
    <tag>_edges       [E,2] int64 (u <= v) sorted, <tag>_length  their 'length' (up to 300 nodes);
    <tag>_edges_sha, <tag>_length_sha   sha256 of those arrays' bytes (every case)
    <tag>_label, <tag>_key   node attributes in node order (strings; up to 700 nodes);
    <tag>_label_sha, <tag>_key_sha      sha256 of the newline-joined strings (every case)
    <tag>_membership  np.packbits of the default-metric neighborhoods (some cases)
    <tag>_next_rand   (seed=None case) np.random.rand() right after loading, the global stream having been
                      seeded with 123 before the load
Only data is written.
"""
import gzip
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = 300                                                         # edge / length arrays stored up to this size
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def geometric_edges(rng, n, degree):
    """Random geometric graph on n uniform points with about `degree` neighbours per node; every node gets at
    least its nearest neighbour, so all n nodes appear in the edge list."""
    xy = rng.uniform(size=(n, 2))
    r = np.sqrt(degree / (np.pi * n))
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    adj = d < r
    nearest = d.argmin(axis=1)
    adj[np.arange(n), nearest] = True
    adj |= adj.T
    iu, ju = np.nonzero(np.triu(adj, k=1))
    order = rng.permutation(iu.size)
    return iu[order], ju[order]


def edge_list_text(rng, n, degree, columns, header, self_loop=False):
    iu, ju = geometric_edges(rng, n, degree)
    relabel = rng.permutation(n)                                  # node numbering != generation order
    rows = []
    if header:
        rows.append('\t'.join(['label1', 'key1', 'label2', 'key2', 'weight'][:columns] if columns == 5
                              else ['key1', 'key2', 'weight']))
    pairs = list(zip(iu.tolist(), ju.tolist()))
    if self_loop:
        pairs.insert(len(pairs) // 2, (int(iu[0]), int(iu[0])))
    for u, v in pairs:
        a, b = relabel[u], relabel[v]
        w = '%.1f' % rng.uniform(0.1, 2.0)
        if columns == 3:
            rows.append('G%05d\tG%05d\t%s' % (a, b, w))
        else:
            rows.append('gene%d\tORF%05d\tgene%d\tORF%05d\t%s' % (a, a, b, b, w))
    return ('\n'.join(rows) + '\n').encode()


def count_iterations(fn):
    """Runs fn() and returns (its result, the number of spring-layout iterations networkx ran): every
    iteration of both of networkx's forms ends in one np.linalg.norm(delta_pos) without an axis."""
    real = np.linalg.norm
    calls = [0]

    def norm(x, *a, **k):
        if not a and k.get('axis') is None:
            calls[0] += 1
        return real(x, *a, **k)
    np.linalg.norm = norm
    try:
        out = fn()
    finally:
        np.linalg.norm = real
    return out, calls[0]


def digest(a):
    """sha256 of an int64 / float64 array's C-order bytes, or of a list of strings joined by newlines."""
    if isinstance(a, list):
        return hashlib.sha256('\n'.join(a).encode()).hexdigest()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(out, tag, G):
    """Coordinates as arrays; edges and lengths as digests, and as arrays too for networks of up to 300 nodes
    (the fixture stays small; a digest is as strict for bit equality)."""
    n = G.number_of_nodes()
    assert list(G) == list(range(n))
    out[tag + '_x'] = np.array([G.nodes[i]['x'] for i in range(n)], dtype=np.float64)
    out[tag + '_y'] = np.array([G.nodes[i]['y'] for i in range(n)], dtype=np.float64)
    edges = sorted((min(u, v), max(u, v), d.get('length', np.nan)) for u, v, d in G.edges(data=True))
    e = np.array([x[:2] for x in edges], dtype=np.int64).reshape(-1, 2)
    length = np.array([x[2] for x in edges], dtype=np.float64)
    out[tag + '_edges_sha'], out[tag + '_length_sha'] = np.array(digest(e)), np.array(digest(length))
    if n <= SMALL:
        out[tag + '_edges'], out[tag + '_length'] = e, length


CASES = [
    # tag, file name, n, mean degree, columns, header, seed, membership, self loop
    ('txt300', 'net300.txt', 300, 12, 3, False, 11, True, True),
    ('tsv700', 'net700.tsv', 700, 15, 5, True, 12, True, False),
    ('gz', 'net250.txt.gz', 250, 10, 3, False, 13, True, False),
    ('n499', 'net499.txt', 499, 10, 3, False, 14, False, False),
    ('n500', 'net500.txt', 500, 10, 3, False, 15, False, False),
    ('tsvgz', 'net520.tsv.gz', 520, 20, 5, True, 16, False, False),
    ('seednone', 'netnone.txt', 150, 10, 3, False, None, False, False),
    ('n1', 'net1.txt', 1, 0, 3, False, 18, False, False),
    ('n2', 'net2.tsv', 2, 0, 5, True, 19, False, False),
    ('big', 'net4000.txt', 4000, 8, 3, False, 17, False, False),
]


def main():
    import warnings
    warnings.simplefilter('ignore')
    safe, _, safe_io = import_reference()
    import networkx as nx
    rng = np.random.default_rng(2024)
    tmp = tempfile.mkdtemp()
    out = {'networkx_version': np.array(nx.__version__)}
    tags = []
    for tag, name, n, degree, columns, header, seed, membership, self_loop in CASES:
        if n == 1:                                                 # one node: its self-loop
            text = b'YAL001C\tYAL001C\t1.0\n'
        elif n == 2:
            text = b'label1\tkey1\tlabel2\tkey2\tweight\nTFC3\tYAL001C\tVPS8\tYAL002W\t0.5\n'
        else:
            text = edge_list_text(rng, n, degree, columns, header, self_loop)
        path = os.path.join(tmp, name)
        with (gzip.open if name.endswith('.gz') else open)(path, 'wb') as f:
            f.write(text)
        out[tag + '_file'] = np.frombuffer(open(path, 'rb').read(), dtype=np.uint8)
        out[tag + '_name'] = np.array(name)
        out[tag + '_seed'] = np.array(-1 if seed is None else seed)
        sf = safe.SAFE(verbose=False)
        sf.random_seed = seed
        t0 = time.time()
        if seed is None:
            np.random.seed(123)
        _, iters = count_iterations(lambda: sf.load_network(network_file=path))
        if seed is None:
            out[tag + '_next_rand'] = np.array(np.random.rand())
        took = time.time() - t0
        G = sf.graph
        record(out, tag, G)
        out[tag + '_iters'] = np.array(iters)
        n_nodes = G.number_of_nodes()
        labels = [str(G.nodes[i]['label']) for i in range(n_nodes)]
        keys = [str(G.nodes[i]['key']) for i in range(n_nodes)]
        out[tag + '_label_sha'], out[tag + '_key_sha'] = np.array(digest(labels)), np.array(digest(keys))
        if n_nodes <= 700:
            out[tag + '_label'], out[tag + '_key'] = np.array(labels), np.array(keys)
        if membership:
            sf.define_neighborhoods()
            out[tag + '_membership'] = np.packbits(np.asarray(sf.neighborhoods, dtype=bool), axis=1)
        print('%-9s N=%5d edges=%6d iterations=%3d  %.1f s' % (tag, n_nodes, G.number_of_edges(), iters, took), flush=True)
        tags.append(tag)

    # weighted in-memory graphs with a self-loop: apply_network_layout directly (f64 and f32 forms)
    for tag, n, seed in (('w60', 60, 21), ('w520', 520, 22)):
        iu, ju = geometric_edges(rng, n, 8)
        w = rng.uniform(0.1, 3.0, size=iu.size).round(3)
        G = nx.Graph()
        G.add_nodes_from(range(n))
        for u, v, x in zip(iu.tolist(), ju.tolist(), w.tolist()):
            G.add_edge(u, v, weight=x)
        G.add_edge(3, 3, weight=2.5)
        out[tag + '_edges_in'] = np.array([(u, v) for u, v in G.edges()], dtype=np.int64)
        out[tag + '_weight_in'] = np.array([d['weight'] for _, _, d in G.edges(data=True)], dtype=np.float64)
        out[tag + '_seed'] = np.array(seed)
        G, iters = count_iterations(lambda: safe_io.apply_network_layout(G, layout='spring_embedded', seed=seed,
                                                                         verbose=False))
        record(out, tag, G)
        out[tag + '_iters'] = np.array(iters)
        print('%-9s N=%5d iterations=%3d' % (tag, n, iters), flush=True)
        tags.append(tag)
    out['tags'] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, 'layout.npz'), **out)
    print('wrote', os.path.join(HERE, 'layout.npz'))


if __name__ == '__main__':
    main()
