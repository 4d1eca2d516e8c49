"""Generates tests/golden/kk.npz: nx.kamada_kawai_layout positions (networkx 3.4.2, NumPy 2.2, SciPy 1.15) of small graphs,
with the edge lists they were computed from.  Calls networkx only.

  python tests/golden/make_kk_golden.py

Cases (key prefix): gnp<n> for n = 1, 2, 3, 50, 130, 300, 600 -- G(n, 4/n), isolated nodes and several components
included; weighted -- 60 nodes, weights 0.1 / 0.3 / 1.7 and a self-loop; twocomp -- two components of 20 and 13 nodes;
txt -- an unweighted edge list as load_network_from_txt reads it (nodes numbered by first appearance: the first column's
labels, then the second's), with the edge lengths of the laid-out graph.
Arrays per case: <case>_u, <case>_v (int32 edges), <case>_w (f64, weighted only), <case>_n, <case>_pos [n, 2] f64."""
import os

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def gnp_edges(n, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(n, 1)
    keep = rng.uniform(size=iu.size) < 4.0 / max(n, 1)
    return iu[keep], ju[keep]


def layout(n, u, v, w=None):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    if w is None:
        G.add_edges_from(zip(u.tolist(), v.tolist()))
    else:
        G.add_weighted_edges_from(zip(u.tolist(), v.tolist(), w.tolist()))
    pos = nx.kamada_kawai_layout(G)
    return np.array([pos[i] for i in range(n)], dtype=np.float64).reshape(n, 2)


def main():
    out = {}

    def add(case, n, u, v, w=None):
        out[case + '_n'] = np.int64(n)
        out[case + '_u'], out[case + '_v'] = np.asarray(u, dtype=np.int32), np.asarray(v, dtype=np.int32)
        if w is not None:
            out[case + '_w'] = np.asarray(w, dtype=np.float64)
        out[case + '_pos'] = layout(n, out[case + '_u'], out[case + '_v'], w)

    for n in (1, 2, 3, 50, 130, 300, 600):
        u, v = gnp_edges(n, 1000 + n)
        if n == 2:
            u, v = np.array([0]), np.array([1])
        add('gnp%d' % n, n, u, v)

    rng = np.random.default_rng(7)
    u, v = gnp_edges(60, 7)
    w = np.array([0.1, 0.3, 1.7])[rng.integers(0, 3, size=u.size)]
    add('weighted', 60, np.append(u, 5), np.append(v, 5), np.append(w, 0.3))       # ... and a self-loop on node 5

    a = nx.gnp_random_graph(20, 0.2, seed=3)
    a.add_edges_from((i, i + 1) for i in range(19))                                 # connected
    b = nx.cycle_graph(13)
    e = list(a.edges()) + [(20 + p, 20 + q) for p, q in b.edges()]
    add('twocomp', 33, [p for p, _ in e], [q for _, q in e])

    # the edge list of a file: labels L<k>, numbered as the loader numbers them
    u, v = gnp_edges(40, 11)
    order = {}
    for lab in list(u.tolist()) + list(v.tolist()):
        order.setdefault(lab, len(order))
    fu, fv = np.array([order[x] for x in u.tolist()]), np.array([order[x] for x in v.tolist()])
    add('txt', len(order), fu, fv)
    pos = out['txt_pos']
    d = pos[fu] - pos[fv]
    out['txt_length'] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    out['txt_labels'] = np.array([lab for lab, _ in sorted(order.items(), key=lambda kv: kv[1])], dtype=np.int32)

    np.savez_compressed(os.path.join(HERE, 'kk.npz'), **out)
    print('wrote kk.npz:', {k: v.shape for k, v in out.items() if k.endswith('_pos')})


if __name__ == '__main__':
    main()
