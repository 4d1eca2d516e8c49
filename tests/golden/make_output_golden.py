#!/usr/bin/env python3
"""Generate tests/golden/output_files.npz by running the REAL reference's print_output_files (safepy/safe.py:1267-1306).

Run in the build container only (needs /root/reference, networkx, pandas; imports the reference like make_golden.py):

    python tests/golden/make_output_golden.py

Two seeded randomization cases of 300 nodes -- randomization only: its NES values are bit-exact on the device path, so the
files must be too -- each stored as its inputs (layout, edges, attributes, names, keys, labels, settings) and the three
files the reference writes, as bytes:

  nes_*      quantitative attributes with NaN rows: node_properties_annotation.txt is the [N, M] NES table
  dom_*      binary attributes, define_top_attributes -> define_domains -> trim_domains first: the domain forms
Only data is written: no reference source travels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import clustered_layout, import_reference, radius_graph_edges   # noqa: E402

FILES = ('domain_properties_annotation.txt', 'attribute_properties_annotation.txt', 'node_properties_annotation.txt')


def keys_labels(n):
    keys = ['ORF%d' % i for i in range(n)]
    labels = ['n%d' % i for i in range(n)]
    keys[7] = 'Y"AL 7'                  # pandas quotes it (QUOTE_MINIMAL)
    labels[11] = 'tab\tlabel'
    return keys, labels


def run_case(safe, safe_io, nx, pd, out_dir, tag, seed, domains):
    rng = np.random.default_rng(seed)
    n, m, nperm, rseed = 300, (40 if domains else 24), 200, 11 + seed
    xy = clustered_layout(rng, n)
    eu, ev = radius_graph_edges(xy, 0.08, rng)
    keys, labels = keys_labels(n)
    g = nx.Graph()
    for i in range(n):
        g.add_node(i, x=float(xy[i, 0]), y=float(xy[i, 1]), key=keys[i], label=labels[i])
    for u, v in zip(eu, ev):
        g.add_edge(int(u), int(v))
    g = safe_io.calculate_edge_lengths(g, verbose=False)
    if domains:
        b = np.zeros((n, m))
        for j in range(m):
            c = xy[rng.integers(n)]
            d = np.sqrt(((xy - c) ** 2).sum(1))
            b[:, j] = (d < rng.uniform(0.05, 0.15)) & (rng.uniform(size=n) < 0.8)
    else:
        b = np.round(rng.standard_normal((n, m)) * 1024) / 1024
        b[rng.choice(n, 15, replace=False)] = np.nan
    names = ['%s %s %d' % (rng.choice(['dna', 'rna', 'protein']), rng.choice(['repair', 'transport', 'folding']), j)
             for j in range(m)]
    names[3] = 'quoted "name" 3'
    sf = safe.SAFE(verbose=False)
    sf.graph = g
    sf.random_seed = rseed
    sf.define_neighborhoods(node_distance_metric='shortpath_weighted_layout', neighborhood_radius=0.2)
    sf.node2attribute = b.copy()
    sf.attributes = pd.DataFrame({'id': np.arange(m), 'name': names})
    sf.compute_pvalues(how='randomization', num_permutations=nperm)
    if domains:
        sf.define_top_attributes()
        sf.define_domains()
        sf.trim_domains()
        assert len(sf.domains) >= 3, 'the case needs at least two domains besides 0'
    case_dir = os.path.join(out_dir, tag)
    os.makedirs(case_dir)
    sf.print_output_files(output_dir=case_dir)
    out = {tag + 'xy': xy, tag + 'edge_u': eu, tag + 'edge_v': ev, tag + 'attributes': b, tag + 'names': np.array(names),
           tag + 'keys': np.array(keys), tag + 'labels': np.array(labels), tag + 'meta': np.array([nperm, rseed, int(domains)])}
    for f in FILES:
        path = os.path.join(case_dir, f)
        data = open(path, 'rb').read() if os.path.exists(path) else b''
        out[tag + f.split('_')[0]] = np.frombuffer(data, dtype=np.uint8)
    return out


def main():
    import tempfile
    import warnings
    warnings.simplefilter('ignore')
    safe, _, safe_io = import_reference()
    import networkx as nx
    import pandas as pd
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        out.update(run_case(safe, safe_io, nx, pd, tmp, 'nes_', 1, False))
        out.update(run_case(safe, safe_io, nx, pd, tmp, 'dom_', 5, True))
    np.savez_compressed(os.path.join(HERE, 'output_files.npz'), **out)


if __name__ == '__main__':
    main()
