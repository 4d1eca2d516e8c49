"""Gene-to-term matrices, the parts that need no device: the OBO / GAF parsers against a hand-written file, the restatement
(tests/go_ref.py) against an example worked out by hand, the refusals, the text file's bytes, and the new symbols in the
header, the binding and the library."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import go_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OBO = """format-version: 1.2
ontology: hand-written

[Term]
id: GO:0000003 ! first in the file
name: child a
namespace: biological_process
is_a: GO:0000001 ! the root, mentioned before its stanza
is_a: GO:0000002 ! a second parent

[Typedef]
id: part_of
name: part of
is_a: GO:0000099 ! not a term

[Term]
id: GO:0000001
name: root process
namespace: biological_process

[Term]
id: GO:0000002
name: mid ! with a comment
namespace: biological_process
is_a: GO:0000001

[Term]
id: GO:0000004
name: obsolete thing
namespace: biological_process
is_a: GO:0000001

[Term]
id: GO:0000005
name: a component
namespace: cellular_component

[Term]
id: GO:0000006
name: a function
namespace: molecular_function
is_a: GO:0000007 ! never defined: takes this term's namespace
"""


def test_parser_on_a_hand_written_file(tmp_path):
    from safepy_amd.utils import make_go
    path = tmp_path / 'hand.obo'
    path.write_text(OBO)
    stanzas = list(make_go.parse_go_obo(str(path)))
    assert [s['id'] for s in stanzas] == ['GO:0000003', 'GO:0000001', 'GO:0000002', 'GO:0000004', 'GO:0000005', 'GO:0000006']
    assert stanzas[0]['is_a'] == ['GO:0000001', 'GO:0000002'] and stanzas[2]['is_a'] == ['GO:0000001']
    assert stanzas[2]['name'] == 'mid' and 'is_a' not in stanzas[1]
    go = make_go.get_go_graph(str(path))
    g = go['go_graph']
    assert g.terms == ['GO:0000003', 'GO:0000001', 'GO:0000002', 'GO:0000005', 'GO:0000006', 'GO:0000007']      # order of first mention
    assert g.edges == [('GO:0000001', 'GO:0000003'), ('GO:0000002', 'GO:0000003'), ('GO:0000001', 'GO:0000002'),
                       ('GO:0000007', 'GO:0000006')]
    assert g.namespace == {'GO:0000003': 'biological_process', 'GO:0000001': 'biological_process', 'GO:0000002': 'biological_process',
                           'GO:0000005': 'cellular_component', 'GO:0000006': 'molecular_function', 'GO:0000007': 'molecular_function'}
    assert 'GO:0000004' not in g.namespace and 'GO:0000099' not in g.namespace and 'part_of' not in g.namespace
    assert list(go['go_details']['id']) == ['GO:0000003', 'GO:0000001', 'GO:0000002', 'GO:0000005', 'GO:0000006']
    assert list(go['go_details'].index) == list(go['go_details']['id'])
    assert go['go_details'].loc['GO:0000002', 'name'] == 'mid'
    p = g.branch('p')
    assert p.terms == ['GO:0000003', 'GO:0000001', 'GO:0000002'] and len(p.edges) == 3 and p.roots() == ['GO:0000001']
    assert g.branch('c').terms == ['GO:0000005'] and g.branch('c').edges == []
    f = g.branch('f')
    assert f.terms == ['GO:0000006', 'GO:0000007'] and f.roots() == ['GO:0000007'] and f.name['GO:0000007'] == 'GO:0000007'


def test_annotation_reader(tmp_path):
    from safepy_amd.utils import make_go
    pairs = [('YAL001C', 'GO:0000003'), ('YBR002W', 'GO:0000002'), ('YAL001C', 'GO:0000003'), ('YCR003W', 'GO:0000001')]
    for name in ('ann.gaf', 'ann.gaf.gz'):
        go_ref.write_gaf(tmp_path / name, pairs)
        table = make_go.read_annotations(str(tmp_path / name))
        assert list(table[1]) == [l for l, _ in pairs] and list(table[4]) == [t for _, t in pairs]
        assert list(table.index) == list(table[1]) and table.shape == (4, 17)
        assert table[3].tolist()[3] == 'NOT|involved_in'          # the qualifier is read and never filtered on


# -------------------------------------------------------------------------------------------- the worked example ----
# eight terms of the process branch and one component; T1 and T2 meet in T3 (a diamond); T5 and T7 have no locus
T = ['GO:000000%d' % k for k in range(8)]
EDGES = [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4), (0, 5), (2, 6), (6, 7)]
ANNOTATIONS = [('a', T[4]), ('b', T[3]), ('c', T[6]), ('d', 'GO:0000100'), ('e', T[1]), ('q', T[2]), ('b', T[3])]
ORDER = ['a', 'b', 'c', 'd', 'zz', 'e']               # zz: unknown to the annotations; q: not listed; d: another branch only
KEPT = [T[0], T[1], T[2], T[3], T[4], T[6]]
BY_HAND = np.array([[1, 1, 1, 1, 1, 0],               # a: T4 and everything above it, through both arms of the diamond
                    [1, 1, 1, 1, 0, 0],               # b: T3, T1, T2, T0
                    [1, 0, 1, 0, 0, 1],               # c: T6, T2, T0
                    [1, 0, 0, 0, 0, 0],               # d: no term in this branch -> the root
                    [0, 0, 0, 0, 0, 0],               # zz: missing, stays empty
                    [1, 1, 0, 0, 0, 0]])              # e: T1, T0


def example_graph():
    from safepy_amd.utils.make_go import GoGraph
    terms = [T[3], T[0], T[1], T[2], T[4], T[5], T[6], T[7], 'GO:0000100']      # some file order; the root is not first
    ns = {t: 'biological_process' for t in T}
    ns['GO:0000100'] = 'cellular_component'
    return GoGraph(terms, ns, {t: 'name of ' + t for t in terms}, [(T[p], T[c]) for p, c in EDGES], set(terms))


def test_restatement_against_the_example_by_hand():
    ref = go_ref.matrix_ref(example_graph(), ANNOTATIONS, 'p', ORDER)
    assert ref['terms'] == KEPT and ref['loci'] == ORDER and ref['root'] == T[0]
    assert np.array_equal(ref['ints'], BY_HAND)
    assert ref['missing'].tolist() == [0, 0, 0, 0, 1, 0] and ref['assigned'] == 1
    assert np.isnan(ref['dense'][4]).all() and np.array_equal(ref['dense'][[0, 1, 2, 3, 5]], BY_HAND[[0, 1, 2, 3, 5]].astype(np.float32))
    # the same through the index form the device entry point takes
    rows = {l: i for i, l in enumerate(ORDER)}
    col = {t: j for j, t in enumerate(T)}
    pairs = [(rows[l], col[t]) for l, t in ANNOTATIONS if l in rows and t in col]
    got = go_ref.closure_ref(6, 8, EDGES, [r for r, _ in pairs], [t for _, t in pairs], 0, missing=[0, 0, 0, 0, 1, 0])
    assert got['kept'].tolist() == [0, 1, 2, 3, 4, 6] and got['assigned'] == 1
    assert got['indptr'].tolist() == [0, 5, 8, 11, 13, 14, 15]
    assert got['indices'].tolist() == [0, 1, 2, 3, 5, 0, 1, 5, 0, 1, 2, 0, 1, 0, 2]
    assert np.array_equal(sp.csc_array((np.ones(15), got['indices'], got['indptr']), shape=(6, 6)).toarray(), BY_HAND)
    ptr, idx = go_ref.children_csr(8, EDGES)
    assert ptr.tolist() == [0, 3, 4, 6, 7, 7, 7, 8, 8] and idx.tolist() == [1, 2, 5, 3, 3, 6, 4, 7]


def test_without_an_order_rows_are_the_files_loci():
    ref = go_ref.matrix_ref(example_graph(), ANNOTATIONS, 'p')
    assert ref['loci'] == ['a', 'b', 'c', 'd', 'e', 'q'] and not ref['missing'].any() and ref['assigned'] == 1
    assert ref['ints'][5].tolist() == [1, 0, 1, 0, 0, 0]                      # q: T2, T0
    assert np.array_equal(ref['ints'][:5], BY_HAND[[0, 1, 2, 3, 5]])


def test_order_with_a_repeated_an_unknown_and_a_dropped_key():
    ref = go_ref.matrix_ref(example_graph(), ANNOTATIONS, 'p', ['b', 'a', 'b', 'nope'])
    assert ref['missing'].tolist() == [0, 0, 0, 1] and ref['assigned'] == 0
    assert ref['terms'] == [T[0], T[1], T[2], T[3], T[4]]                     # T6 had only c, which is not listed
    assert np.array_equal(ref['ints'][0], ref['ints'][2]) and ref['ints'][0].tolist() == [1, 1, 1, 1, 0]
    assert ref['ints'][1].tolist() == [1, 1, 1, 1, 1] and ref['ints'][3].tolist() == [0, 0, 0, 0, 0]


@pytest.mark.parametrize('seed', [0, 1])
def test_on_a_tree_ancestors_are_the_parent_chain(seed):
    rng = np.random.default_rng(seed)
    n_terms, n_rows = 60, 40
    edges = go_ref.random_dag(rng, n_terms, 7, max_parents=1)
    parent = {c: p for p, c in edges}
    assert len(parent) == n_terms - 1                                         # one parent each: a tree
    ann_row, ann_term = rng.integers(0, n_rows, 80), rng.integers(0, n_terms, 80)
    want = np.zeros((n_rows, n_terms), dtype=np.uint8)
    for r, t in zip(ann_row.tolist(), ann_term.tolist()):
        while True:
            want[r, t] = 1
            if t not in parent:
                break
            t = parent[t]
    lonely = want.sum(axis=1) == 0
    want[lonely, 0] = 1
    got = go_ref.closure_ref(n_rows, n_terms, edges, ann_row, ann_term, 0)
    assert np.array_equal(got['dense'], want) and got['assigned'] == int(lonely.sum())


def test_matrix_txt_bytes_against_pandas(tmp_path):
    import pandas as pd
    from safepy_amd.utils.make_go import GoMatrix
    loci = ORDER[:3] + ['tab\there', 'quote"d'] + ORDER[5:]                   # labels the writer has to quote
    gm = GoMatrix(loci, KEPT, None, sp.csc_array(BY_HAND.astype(np.float32)), np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8), 1, loci, T[0], None)
    gm.write_txt(str(tmp_path / 'go_p_matrix.txt'), block_rows=4)
    want = pd.DataFrame(BY_HAND.astype(int), index=loci, columns=KEPT).to_csv(sep='\t')
    assert (tmp_path / 'go_p_matrix.txt').read_bytes() == want.encode('utf-8')
    frame = gm.to_frame()
    assert list(frame.index) == loci and list(frame.columns) == KEPT and np.array_equal(frame.to_numpy(), BY_HAND)
    assert all(isinstance(d, pd.SparseDtype) for d in frame.dtypes)


def test_refusals_write_nothing(tmp_path):
    from safepy_amd.utils import make_go
    go_ref.write_gaf(tmp_path / 'ann.gaf', [('a', go_ref.term_id(1))])
    # a cycle among the branch's edges
    go_ref.write_obo(tmp_path / 'cycle.obo', 4, [(0, 1), (1, 2), (2, 3), (3, 1)])
    with pytest.raises(ValueError, match='cycle'):
        make_go.make_go_matrix(str(tmp_path / 'cycle.obo'), str(tmp_path / 'ann.gaf'), 'p')
    # an is_a to an id that no stanza defines, from a term that has no namespace to hand down
    (tmp_path / 'orphan.obo').write_text('[Term]\nid: GO:0000001\nname: nameless space\nis_a: GO:0000777\n\n'
                                         '[Term]\nid: GO:0000002\nname: fine\nnamespace: biological_process\n')
    with pytest.raises(ValueError, match='GO:0000777'):
        make_go.make_go_matrix(str(tmp_path / 'orphan.obo'), str(tmp_path / 'ann.gaf'), 'p')
    # a branch with no term
    go_ref.write_obo(tmp_path / 'only_p.obo', 3, [(0, 1), (0, 2)])
    with pytest.raises(ValueError, match='no term'):
        make_go.make_go_matrix(str(tmp_path / 'only_p.obo'), str(tmp_path / 'ann.gaf'), 'c')
    with pytest.raises(ValueError, match='go_branch'):
        make_go.make_go_matrix(str(tmp_path / 'only_p.obo'), str(tmp_path / 'ann.gaf'), 'x')
    assert sorted(os.listdir(tmp_path)) == ['ann.gaf', 'cycle.obo', 'only_p.obo', 'orphan.obo']


def test_load_attributes_refuses_a_matrix_in_another_row_order():
    import safepy_amd
    from safepy_amd.utils.make_go import GoMatrix
    m = sp.csc_array(BY_HAND.astype(np.float32))
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = safepy_amd.LayoutGraph(np.random.default_rng(0).uniform(size=(6, 2)), keys=list(ORDER))
    details = {'id': KEPT, 'name': ['n%d' % k for k in range(6)]}
    import pandas as pd
    for loci, order in ((ORDER, None), (ORDER[::-1], ORDER[::-1])):           # built without an order; built in another order
        gm = GoMatrix(list(loci), KEPT, pd.DataFrame(details), m, np.zeros(6, dtype=np.uint8), 0, order, T[0], None)
        with pytest.raises(ValueError, match='node_label_order'):
            sf.load_attributes(attribute_file=gm)
    gm = GoMatrix(list(ORDER), KEPT, pd.DataFrame(details), m, np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8), 1, list(ORDER), T[0], None)
    sf.load_attributes(attribute_file=gm)                                     # (no device work without keep_on_device)
    assert sf.node2attribute is m and sf._missing_rows.tolist() == [0, 0, 0, 0, 1, 0]
    assert sf.attributes['id'].tolist() == KEPT and sf.attributes['name'].tolist() == details['name']


def test_a_loaded_matrix_pickles_without_its_device_part():
    """SAFE keeps the GoMatrix as its attribute source; the device handle behind it (a ctypes pointer) must not reach pickle."""
    import ctypes
    import pickle
    import pandas as pd
    import safepy_amd
    from safepy_amd.utils.make_go import GoMatrix

    class Held:                                                               # stands in for backend.GoClosure: a live handle
        def __init__(self):
            self.handle, self.ctx, self.closed = ctypes.c_void_p(0x1000), None, False

        def close(self):
            self.handle, self.closed = None, True
    with pytest.raises(ValueError):
        pickle.dumps(Held().handle)                                           # (what the handle does to pickle if it gets there)
    held = Held()
    m = sp.csc_array(BY_HAND.astype(np.float32))
    gm = GoMatrix(list(ORDER), KEPT, pd.DataFrame({'id': KEPT, 'name': KEPT}), m, np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8), 1,
                  list(ORDER), T[0], held)
    assert gm.on_device
    sf = safepy_amd.SAFE(verbose=False)
    sf.graph = safepy_amd.LayoutGraph(np.random.default_rng(0).uniform(size=(6, 2)), keys=list(ORDER))
    sf.load_attributes(attribute_file=gm)
    assert sf.path_to_attribute_file is gm
    back = pickle.loads(pickle.dumps(sf))
    assert gm.on_device and not held.closed                                   # pickling took nothing from the original
    assert not back.path_to_attribute_file.on_device
    assert np.array_equal(back.node2attribute.toarray(), BY_HAND) and back.attributes['id'].tolist() == KEPT
    copy = pickle.loads(pickle.dumps(gm))
    assert not copy.on_device and copy.terms == KEPT and copy.loci == ORDER and copy.missing_rows.tolist() == [0, 0, 0, 0, 1, 0]
    assert np.array_equal(copy.matrix.toarray(), BY_HAND) and copy.num_root_assigned == 1
    gm.release()
    assert held.closed and not gm.on_device


def test_symbols_are_declared_bound_and_exported():
    from safepy_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    want = {'safe_go_create': 15, 'safe_go_read': 5, 'safe_go_as_attr': 2, 'safe_go_pass_ms': 3, 'safe_go_destroy': 1}
    for name, n_args in want.items():
        found = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, code)
        assert found, name
        assert len(found.group(1).split(',')) == n_args, name
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == n_args, name
        assert hasattr(_lib.lib, name), name
    assert re.search(r'typedef\s+struct\s+safe_go\s+safe_go\s*;', code)
    version = int(re.search(r'#define SAFE_HIP_ABI_VERSION (\d+)', header).group(1))
    assert version == _lib.ABI_VERSION == _lib.lib.safe_abi_version()
    makefile = open(os.path.join(ROOT, 'safepy_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRC\s*:=.*\bgo\.hip\b', makefile, flags=re.M)
    from safepy_amd import backend
    assert all(hasattr(backend.GoClosure, m) for m in ('read', 'as_attributes', 'close', 'pass_ms'))
