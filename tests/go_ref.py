"""NumPy / networkx restatement of the gene-to-term matrix (safepy_amd/utils/make_go.py, csrc/go.hip) and a seeded generator
of synthetic ontologies and annotation files.  Checker only: nothing here is imported by the package.

The contract restated ("a matrix of gene-to-term annotations (propagated)"): cell (locus, term) = 1 iff the locus is annotated
to the term or to any descendant of it -- the term itself plus nx.ancestors(term) of every directly annotated term; then terms
without a locus are dropped; then every non-missing locus without a term is given to the root."""
import gzip

import networkx as nx
import numpy as np

NAMESPACES = {'p': 'biological_process', 'c': 'cellular_component', 'f': 'molecular_function'}


def closure_ref(n_rows, n_terms, edges, ann_row, ann_term, root, missing=None):
    """edges: (parent, child) index pairs.  Returns dict(dense u8 [n_rows, n_terms] AFTER the root rule and BEFORE the drop,
    kept, indptr int64, indices int32, assigned)."""
    g = nx.DiGraph()
    g.add_nodes_from(range(n_terms))
    g.add_edges_from((int(p), int(c)) for p, c in edges)
    dense = np.zeros((n_rows, n_terms), dtype=np.uint8)
    ann_row, ann_term = np.asarray(ann_row, dtype=np.int64), np.asarray(ann_term, dtype=np.int64)
    for t in np.unique(ann_term).tolist():
        rows = ann_row[ann_term == t]
        up = np.array(sorted(nx.ancestors(g, t) | {t}), dtype=np.int64)
        dense[np.ix_(rows, up)] = 1
    kept = dense.sum(axis=0) > 0                                     # terms with zero loci are dropped ...
    lonely = dense[:, kept].sum(axis=1) == 0                         # ... then loci with zero remaining terms
    if missing is not None:
        lonely &= np.asarray(missing) == 0
    dense[lonely, root] = 1                                          # go to the root, whose column is kept if it has any locus now
    kept = dense.sum(axis=0) > 0
    kept_idx = np.flatnonzero(kept).astype(np.int32)
    cols = dense[:, kept_idx]
    indptr = np.zeros(kept_idx.shape[0] + 1, dtype=np.int64)
    np.cumsum(cols.sum(axis=0, dtype=np.int64), out=indptr[1:])
    indices = np.nonzero(cols.T)[1].astype(np.int32)                 # column by column, rows ascending
    return dict(dense=dense, kept=kept_idx, indptr=indptr, indices=indices, assigned=int(lonely.sum()))


def children_csr(n_terms, edges):
    """(child_ptr int32 [n_terms + 1], child_idx int32) of (parent, child) index pairs."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    order = np.argsort(e[:, 0], kind='stable')
    ptr = np.zeros(n_terms + 1, dtype=np.int32)
    np.cumsum(np.bincount(e[:, 0], minlength=n_terms), out=ptr[1:])
    return ptr, e[order, 1].astype(np.int32)


def matrix_ref(parsed, annotations, go_branch, node_label_order=None):
    """The whole restatement from a parse result: parsed = get_go_graph(...)['go_graph'] (terms in file order, namespace,
    edges), annotations = (locus, term) string pairs of the whole file.  Returns dict(loci, terms (kept, sorted), dense f32
    [loci, kept terms] with NaN across missing rows, missing u8, assigned, root)."""
    ns = NAMESPACES[go_branch]
    inside = [t for t in parsed.terms if parsed.namespace.get(t) == ns]
    if not inside:
        raise ValueError('empty branch')
    keep = set(inside)
    g = nx.DiGraph()
    g.add_nodes_from(inside)
    g.add_edges_from((p, c) for p, c in parsed.edges if p in keep and c in keep)
    if not nx.is_directed_acyclic_graph(g):
        raise ValueError('cycle')
    root = [t for t in inside if g.in_degree(t) == 0][0]
    terms = sorted(inside)
    col = {t: j for j, t in enumerate(terms)}
    file_loci = sorted({l for l, _ in annotations})
    loci = file_loci if node_label_order is None else list(node_label_order)
    known = set(file_loci)
    missing = np.array([l not in known for l in loci], dtype=np.uint8)
    rows_of = {}
    for i, l in enumerate(loci):
        rows_of.setdefault(l, []).append(i)
    dense = np.zeros((len(loci), len(terms)), dtype=np.uint8)
    for l, t in annotations:
        if t in keep and l in rows_of:
            for u in nx.ancestors(g, t) | {t}:
                dense[rows_of[l], col[u]] = 1
    kept = dense.sum(axis=0) > 0
    lonely = (dense[:, kept].sum(axis=1) == 0) & (missing == 0)
    dense[lonely, col[root]] = 1
    kept = dense.sum(axis=0) > 0
    out = dense[:, kept].astype(np.float32)
    out[missing != 0] = np.nan
    return dict(loci=loci, terms=[t for t, k in zip(terms, kept) if k], dense=out, ints=dense[:, kept].astype(np.int64), missing=missing,
                assigned=int(lonely.sum()), root=root)


# ------------------------------------------------------------------------------------------------------ generators ----

def random_dag(rng, n_terms, n_levels, max_parents=3):
    """(parent, child) index pairs of a layered DAG: term 0 is the only root, every other term has 1 .. max_parents parents
    on shallower levels (at least one on the level right above, so the depth is n_levels).  Indices are shuffled so that a
    term's index says nothing about its level."""
    n_levels = max(1, min(n_levels, n_terms))
    depth = np.zeros(n_terms, dtype=np.int64)
    if n_terms > 1:
        depth[1:n_levels] = np.arange(1, n_levels)                 # every level is inhabited
        if n_terms > n_levels:
            depth[n_levels:] = rng.integers(1, max(n_levels, 2), size=n_terms - n_levels)
    by_depth = [np.flatnonzero(depth == d) for d in range(n_levels)]
    shallower = [np.flatnonzero(depth < d) for d in range(n_levels)]
    edges = []
    for t in range(1, n_terms):
        d = int(depth[t])
        parents = {int(rng.choice(by_depth[d - 1]))}
        for _ in range(int(rng.integers(0, max_parents))):
            parents.add(int(rng.choice(shallower[d])))
        edges.extend((p, t) for p in sorted(parents))
    relabel = np.concatenate([[0], 1 + rng.permutation(n_terms - 1)]) if n_terms > 1 else np.array([0])
    return [(int(relabel[p]), int(relabel[c])) for p, c in edges]


def term_id(k):
    return 'GO:%07d' % k


def write_obo(path, n_terms, edges, namespace='biological_process', rng=None, extra=''):
    """One [Term] stanza per term, in a shuffled order when rng is given (parents are then often mentioned before their stanza)."""
    parents = {}
    for p, c in edges:
        parents.setdefault(c, []).append(p)
    order = list(range(n_terms)) if rng is None else [0] + (1 + rng.permutation(n_terms - 1)).tolist()
    with open(path, 'w') as f:
        f.write('format-version: 1.2\nontology: synthetic\n\n')
        for t in order:
            f.write('[Term]\nid: %s\nname: term %d\nnamespace: %s\n' % (term_id(t), t, namespace))
            for p in parents.get(t, []):
                f.write('is_a: %s ! term %d\n' % (term_id(p), p))
            f.write('\n')
        f.write(extra)


def write_gaf(path, pairs, other=()):
    """pairs: (locus, term id) strings of the branch; other: further rows (annotations in other branches).  17 GAF columns."""
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(path, 'wt') as f:
        f.write('!gaf-version: 2.2\n!generated for a test\n')
        for k, (locus, term) in enumerate(list(pairs) + list(other)):
            qualifier = 'NOT|involved_in' if k % 7 == 3 else 'involved_in'
            f.write('\t'.join(['DB', locus, locus.lower(), qualifier, term, 'REF:1', 'IEA', '', 'P', '', '', 'gene', 'taxon:1',
                               '20200101', 'DB', '', '']) + '\n')


def synthetic_files(folder, seed, n_terms, n_loci, n_rows, n_levels=8, unannotated=5, elsewhere=4):
    """Writes onto.obo and ann.gaf into folder: a random DAG, n_rows annotation rows over n_loci loci, `unannotated` loci that
    appear only with a term of ANOTHER branch (they go to the root) -- `elsewhere` such rows for annotated loci too.
    Terms whose index ends in 9 get no direct annotation.  Returns (obo path, gaf path, sorted loci of the file)."""
    rng = np.random.default_rng(seed)
    edges = random_dag(rng, n_terms, n_levels)
    other = '[Term]\nid: GO:9000001\nname: a function\nnamespace: molecular_function\n\n'
    obo, gaf = str(folder / 'onto.obo'), str(folder / 'ann.gaf')
    write_obo(obo, n_terms, edges, rng=rng, extra=other)
    names = ['L%05d' % i for i in range(n_loci)]
    body = names[:n_loci - unannotated]
    picks = np.concatenate([np.arange(len(body)), rng.integers(0, len(body), max(n_rows - len(body), 0))])   # every locus at least once
    drawn = rng.integers(0, n_terms, picks.shape[0])
    drawn = np.where(drawn % 10 == 9, drawn - 1, drawn)              # terms 9, 19, ... are never annotated: the leaves among them drop out
    pairs = [(body[int(l)], term_id(int(t))) for l, t in zip(picks, drawn)]
    others = [(l, 'GO:9000001') for l in names[n_loci - unannotated:]] + [(body[int(l)], 'GO:9000001') for l in rng.integers(0, len(body), elsewhere)]
    write_gaf(gaf, pairs, others)
    return obo, gaf, sorted(set(l for l, _ in pairs + others))
