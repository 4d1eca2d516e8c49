"""OBO ontology + GAF annotations -> the propagated gene-to-term matrix SAFE.load_attributes takes (the counterpart of
safepy/utils/make_go.py, whose stated result is "a matrix of gene-to-term annotations (propagated)").

Host (this file): parsing, the choice of the branch, the order of loci and terms, the files.  Device (csrc/go.hip through
backend.GoClosure): the propagation of every direct annotation to all ancestors of its term, the drop of empty terms, the
assignment of loci without a term to the root, and the compaction into CSC.  No dense matrix exists on the host unless
`write_files=True` asks for the tab-separated text, which is written in row blocks.

Semantics ("Gene-to-term matrices"):
  parsing      OBO v1.2 [Term] stanzas; [Typedef] stanzas are skipped; the value of a `key: value` line is the text before
               the first `!`, stripped; terms whose name starts with `obsolete` are skipped; edges are `is_a` only, parent ->
               child; a parent first met in a child's is_a takes that child's namespace; file order = order of first mention
               (as the id of a non-obsolete term or as one of its is_a values)
  branch       go_branch p / c / f: the terms of that namespace and the edges among them
  annotations  tab-separated, lines starting with `!` ignored, 0-based column 1 the locus, column 4 the term; every row
               counts whatever its qualifier says; .gz accepted
  loci         without node_label_order: the sorted distinct loci of the whole file (all branches); with it: that list in
               that order -- a key listed twice gets identical rows, keys the file does not know are `missing_rows`, loci not
               listed are dropped
  matrix       columns = the branch's terms, sorted; cell = 1 iff the locus is annotated to the term or any descendant;
               then terms without a locus are dropped; then every non-missing locus without a term goes to the root (the
               first term in file order without a parent inside the branch), whose column stays in its sorted place
  refusals     ValueError, before anything is written: a cycle among the branch's edges, an is_a to an id that no stanza
               defines and that got no namespace, a branch without a term

usage: python -m safepy_amd.utils.make_go --path-to-obo go-basic.obo --path-to-annotations sgd.gaf.gz --go-branch p"""
import argparse
import csv
import gzip
import logging
import os
import pickle

import numpy as np

NAMESPACES = {'p': 'biological_process', 'c': 'cellular_component', 'f': 'molecular_function'}


def _open_text(path):
    if str(path).endswith('.gz'):
        return gzip.open(path, 'rt', encoding='utf-8', newline='')
    return open(path, 'r', encoding='utf-8', newline='')


def parse_go_obo(path_to_obo):
    """Yields one dict per [Term] stanza, in file order: key -> value, or a list of values for a key given several times;
    `is_a` is always a list.  Lines outside a [Term] stanza (the header, [Typedef] stanzas) yield nothing."""
    def finish(pairs):
        term = {}
        for key, value in pairs:
            term.setdefault(key, []).append(value)
        return {k: (v if k == 'is_a' or len(v) > 1 else v[0]) for k, v in term.items()}

    pairs = None
    with _open_text(path_to_obo) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith('[') and line.endswith(']'):
                if pairs is not None:
                    yield finish(pairs)
                pairs = [] if line == '[Term]' else None
                continue
            if pairs is None:
                continue
            key, _, value = line.partition(':')
            pairs.append((key.strip(), value.partition('!')[0].strip()))
    if pairs is not None:
        yield finish(pairs)


class GoGraph:
    """The is_a graph: `terms` in file order, `namespace[term]`, `name[term]` (the id where no stanza gave one), `edges` as
    (parent, child) in file order without repeats, `defined` = the ids that have a stanza of their own."""

    def __init__(self, terms, namespace, name, edges, defined):
        self.terms, self.namespace, self.name, self.edges, self.defined = list(terms), dict(namespace), dict(name), list(edges), set(defined)

    def branch(self, go_branch):
        """The terms of namespace p / c / f and the edges among them."""
        if go_branch not in NAMESPACES:
            raise ValueError("go_branch must be 'p', 'c' or 'f', got %r" % (go_branch,))
        ns = NAMESPACES[go_branch]
        inside = {t for t in self.terms if self.namespace.get(t) == ns}
        if not inside:
            raise ValueError('the ontology has no term in the %s branch (%s)' % (go_branch, ns))
        return GoGraph([t for t in self.terms if t in inside], {t: ns for t in inside}, {t: self.name[t] for t in inside},
                       [(p, c) for p, c in self.edges if p in inside and c in inside], self.defined & inside)

    def roots(self):
        """Terms without a parent among the graph's edges, in file order."""
        has_parent = {c for _, c in self.edges}
        return [t for t in self.terms if t not in has_parent]

    def check_acyclic(self):
        children = {}
        waiting = dict.fromkeys(self.terms, 0)
        for p, c in self.edges:
            children.setdefault(p, []).append(c)
            waiting[c] += 1
        ready = [t for t in self.terms if waiting[t] == 0]
        done = 0
        while ready:
            t = ready.pop()
            done += 1
            for c in children.get(t, ()):
                waiting[c] -= 1
                if waiting[c] == 0:
                    ready.append(c)
        if done != len(self.terms):
            stuck = [t for t in self.terms if waiting[t] > 0]
            raise ValueError('the is_a edges hold a cycle (among %d terms, e.g. %s)' % (len(stuck), ', '.join(stuck[:3])))


def get_go_graph(path_to_obo):
    """{'go_graph': GoGraph, 'go_details': DataFrame [id, name, namespace] of the non-obsolete stanzas, indexed by id}."""
    import pandas as pd
    terms, namespace, name, edges, defined = [], {}, {}, [], set()
    seen_edges = set()
    details = []

    def mention(term, ns):
        if term not in namespace:
            terms.append(term)
            namespace[term] = ns

    for stanza in parse_go_obo(path_to_obo):
        label = stanza.get('name', '')
        if isinstance(label, list):
            label = label[0]
        if label.startswith('obsolete'):
            continue
        tid = stanza.get('id')
        if isinstance(tid, list):
            tid = tid[0]
        if not tid:
            continue
        ns = stanza.get('namespace')
        if isinstance(ns, list):
            ns = ns[0]
        mention(tid, ns)
        if namespace[tid] is None:                      # (met before as a parent of a term without a namespace)
            namespace[tid] = ns
        defined.add(tid)
        name[tid] = label
        details.append((tid, label, ns))
        for parent in stanza.get('is_a', []):
            mention(parent, ns)
            if (parent, tid) not in seen_edges:
                seen_edges.add((parent, tid))
                edges.append((parent, tid))
    for t in terms:
        if t not in defined and namespace[t] is None:
            raise ValueError('is_a names %s, which no [Term] stanza defines and which has no namespace' % t)
        name.setdefault(t, t)
    go_details = pd.DataFrame(details, columns=['id', 'name', 'namespace'])
    go_details.index = go_details['id'].values
    return {'go_graph': GoGraph(terms, namespace, name, edges, defined), 'go_details': go_details}


def read_annotations(path_to_annotations):
    """The annotation rows as a DataFrame of strings with integer column labels (1 = locus, 4 = term), indexed by locus."""
    import pandas as pd
    rows = []
    with _open_text(path_to_annotations) as f:
        for line in f:
            if line.startswith('!'):
                continue
            line = line.rstrip('\r\n')
            if not line:
                continue
            fields = line.split('\t')
            if len(fields) < 5:
                raise ValueError('annotation row with %d tab-separated fields (at least 5 expected): %r' % (len(fields), line[:80]))
            rows.append(fields)
    width = max((len(r) for r in rows), default=5)
    table = pd.DataFrame([r + [''] * (width - len(r)) for r in rows], columns=list(range(width)), dtype=object)
    table.index = table[1].values
    return table


class GoMatrix:
    """What make_go_matrix returns.
      loci               row labels (node_label_order as given, or the sorted distinct loci of the annotation file)
      terms              ids of the kept terms, sorted: the column labels
      go_details         DataFrame [id, name, namespace] of the kept terms, in column order
      matrix             scipy.sparse.csc_array [len(loci), len(terms)], float32, every stored value 1 (the dtype
                         Attributes.from_sparse uploads without a copy)
      missing_rows       uint8 [len(loci)]: 1 = the annotation file does not know this locus (its row is empty here, NaN
                         on the device)
      num_root_assigned  loci that had no term and were given to the root
      node_label_order   the list the rows follow, or None
      to_attributes(ctx) the f32 device matrix
    The object also keeps the CSC that the device call left on the device (at GO size about 80 MB), so that to_attributes
    expands it there; `on_device` says whether it is still held, `release()` frees it, and so does the end of the object's
    life -- a SAFE instance that loaded the object refers to it as its attribute source.  Pickling (SAFE.save) leaves the
    device part behind: a loaded copy has `on_device == False` and uploads the stored entries of `matrix` instead."""

    def __init__(self, loci, terms, go_details, matrix, missing_rows, num_root_assigned, node_label_order, root, closure):
        self.loci, self.terms, self.go_details, self.matrix = loci, terms, go_details, matrix
        self.missing_rows, self.num_root_assigned, self.node_label_order, self.root = missing_rows, num_root_assigned, node_label_order, root
        self._closure = closure

    @property
    def on_device(self):
        """True while the CSC of the device call is still held: to_attributes(ctx) of that context expands it in place."""
        return self._closure is not None and bool(self._closure.handle)

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_closure'] = None                        # (a device handle: it does not travel)
        return state

    def to_attributes(self, ctx=None):
        """A device handle (backend.Attributes) of the matrix, NaN across missing_rows: expanded from the CSC the closure left
        on the device while that is still there and on `ctx`'s device, else from the stored entries of `matrix`."""
        from .. import backend as be
        c = self._closure
        if c is not None and c.handle and (ctx is None or ctx is c.ctx):
            return c.as_attributes()
        if ctx is None:
            ctx = be.Context.default(0)
        return be.Attributes.from_sparse(ctx, self.matrix, self.missing_rows)

    def release(self):
        """Frees the CSC on the device (to_attributes then uploads the stored entries of `matrix`)."""
        if self._closure is not None:
            self._closure.close()
            self._closure = None

    def to_frame(self):
        """The reference's go_matrix: a pandas DataFrame of integers with sparse columns."""
        import pandas as pd
        return pd.DataFrame.sparse.from_spmatrix(self.matrix.astype(np.int64), index=self.loci, columns=self.terms)

    def write_txt(self, path, block_rows=512):
        """The bytes of pandas.DataFrame(dense int matrix, index=loci, columns=terms).to_csv(path, sep='\\t')."""
        digits = np.array(['0', '1'])
        rows = self.matrix.tocsr()
        with open(path, 'w', encoding='utf-8', newline='') as f:
            w = csv.writer(f, delimiter='\t', lineterminator=os.linesep, quoting=csv.QUOTE_MINIMAL)
            w.writerow([''] + [str(t) for t in self.terms])
            for r0 in range(0, len(self.loci), block_rows):
                block = digits[(rows[r0:r0 + block_rows].toarray() != 0).astype(np.intp)].tolist()
                w.writerows([str(self.loci[r0 + i])] + line for i, line in enumerate(block))


def make_locus2term(go_graph, go_annotations, node_label_order=None, device=0):
    """go_graph: the GoGraph of ONE branch (GoGraph.branch); go_annotations: read_annotations' table.  Returns a GoMatrix;
    the propagation, the two rules and the compaction run on `device`."""
    import pandas as pd
    import scipy.sparse as sp
    from .. import backend as be
    if not go_graph.terms:
        raise ValueError('the branch has no term')
    go_graph.check_acyclic()
    terms = sorted(go_graph.terms)
    term_index = pd.Index(terms)
    roots = go_graph.roots()
    root = roots[0]
    # children of every term, CSR over the sorted terms
    pairs = np.array([(term_index.get_loc(p), term_index.get_loc(c)) for p, c in go_graph.edges], dtype=np.int64).reshape(-1, 2)
    by_parent = np.argsort(pairs[:, 0], kind='stable')
    child_idx = pairs[by_parent, 1].astype(np.int32)
    child_ptr = np.zeros(len(terms) + 1, dtype=np.int32)
    np.cumsum(np.bincount(pairs[:, 0], minlength=len(terms)), out=child_ptr[1:])
    # rows
    ann_loci = go_annotations[1].astype(str).values if len(go_annotations) else np.empty(0, dtype=object)
    ann_terms = go_annotations[4].astype(str).values if len(go_annotations) else np.empty(0, dtype=object)
    if node_label_order is None:
        loci = sorted(set(ann_loci.tolist()))
        order = None
    else:
        order = list(node_label_order)
        loci = order
    if not loci:
        raise ValueError('no locus: the annotation file is empty and no node_label_order was given')
    known = set(ann_loci.tolist())
    missing = np.array([str(k) not in known for k in loci], dtype=np.uint8)
    tcode = term_index.get_indexer(ann_terms) if len(ann_terms) else np.empty(0, dtype=np.int64)
    direct = pd.DataFrame({'locus': ann_loci[tcode >= 0], 'term': tcode[tcode >= 0]}).drop_duplicates()
    rows_of = pd.DataFrame({'locus': [str(k) for k in loci], 'row': np.arange(len(loci), dtype=np.int64)})
    direct = direct.merge(rows_of, on='locus', how='inner')
    ctx = be.Context.default(device)
    closure = be.GoClosure(ctx, len(loci), len(terms), child_ptr, child_idx, direct['row'].values, direct['term'].values,
                           term_index.get_loc(root), missing if missing.any() else None)
    indptr, indices, kept, assigned = closure.read()
    # (nnz is below 2^31, so the pointer array fits the int32 of the row indices: SciPy keeps one index type)
    matrix = sp.csc_array((np.ones(indices.shape[0], dtype=np.float32), indices, indptr.astype(np.int32)), shape=(len(loci), kept.shape[0]))
    kept_terms = [terms[k] for k in kept.tolist()]
    go_details = pd.DataFrame({'id': kept_terms, 'name': [go_graph.name[t] for t in kept_terms],
                               'namespace': [go_graph.namespace[t] for t in kept_terms]})
    logging.info('%d loci had 0 terms and were assigned to the root.' % assigned)
    return GoMatrix(loci, kept_terms, go_details, matrix, missing, int(assigned), order, root, closure)


def make_go_matrix(path_to_obo='', path_to_annotations='', go_branch='p', node_label_order=None, write_files=True, device=0):
    """Builds the propagated gene-to-term matrix of one GO branch (see the module text).  write_files=True also writes, next to
    the annotation file, go_<branch>.p (a pickle of {'go_matrix', 'go_details', 'locus_details', 'tree_path',
    'annotations_path'}, go_matrix a DataFrame with sparse columns) and go_<branch>_matrix.txt (tab-separated 0/1)."""
    go = get_go_graph(path_to_obo)
    branch = go['go_graph'].branch(go_branch)
    branch.check_acyclic()
    annotations = read_annotations(path_to_annotations)
    result = make_locus2term(branch, annotations, node_label_order=node_label_order, device=device)
    if write_files:
        folder = os.path.dirname(path_to_annotations)
        pickle_path = os.path.join(folder, 'go_' + go_branch + '.p')
        logging.info('Saving the results at %s' % pickle_path)
        with open(pickle_path, 'wb') as f:
            pickle.dump({'go_matrix': result.to_frame(), 'go_details': go['go_details'], 'locus_details': annotations,
                         'tree_path': path_to_obo, 'annotations_path': path_to_annotations}, f)
        txt_path = os.path.join(folder, 'go_' + go_branch + '_matrix.txt')
        logging.info('Printing the gene-to-term matrix at %s' % txt_path)
        result.write_txt(txt_path)
    return result


def main(argv=None):
    parser = argparse.ArgumentParser(description='Generate a new matrix of genes (loci) to GO term associations.')
    parser.add_argument('--path-to-obo', type=str, required=True, help='Path to file containing the GO tree')
    parser.add_argument('--path-to-annotations', type=str, required=True, help='Path to gene-to-term annotation file')
    parser.add_argument('--go-branch', default='p', type=str, help='p, c or f')
    args = parser.parse_args(argv)
    make_go_matrix(path_to_obo=args.path_to_obo, path_to_annotations=args.path_to_annotations, go_branch=args.go_branch)


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    main()
