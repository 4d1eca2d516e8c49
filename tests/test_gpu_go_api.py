"""OBO + GAF -> make_go_matrix -> SAFE.load_attributes -> compute_pvalues on generated files (300 terms x 500 loci), against
the restatement of tests/go_ref.py: the matrix is equal, and the hypergeometric results are bit-equal to the same call on the
restatement's dense f32 matrix.  Needs an MI355X."""
import os
import pickle

import numpy as np
import pytest

import go_ref

pytestmark = pytest.mark.gpu

N_TERMS, N_LOCI, N_NODES = 300, 500, 500


@pytest.fixture(scope='module')
def amd():
    import safepy_amd
    assert safepy_amd.device_count() >= 1, 'no HIP device: the GPU tests must run on the MI355X box'
    return safepy_amd


@pytest.fixture(scope='module')
def case(amd, tmp_path_factory):
    """The files, the node keys of the network (497 loci of the file in a shuffled order, one of them twice, two keys the file
    does not know), the GoMatrix in node order and the restatement -- made once."""
    from safepy_amd.utils import make_go
    folder = tmp_path_factory.mktemp('go')
    obo, gaf, loci = go_ref.synthetic_files(folder, 3, N_TERMS, N_LOCI, 2000)
    assert len(loci) == N_LOCI
    rng = np.random.default_rng(4)
    keys = [loci[i] for i in rng.permutation(N_LOCI)[:N_NODES - 3]]
    keys.insert(100, keys[7])
    keys.insert(250, 'not-in-the-file-1')
    keys.append('not-in-the-file-2')
    assert len(keys) == N_NODES
    gm = make_go.make_go_matrix(obo, gaf, 'p', node_label_order=keys, write_files=False)
    parsed = make_go.get_go_graph(obo)['go_graph']
    table = make_go.read_annotations(gaf)
    ref = go_ref.matrix_ref(parsed, list(zip(table[1], table[4])), 'p', keys)
    xy = rng.uniform(size=(N_NODES, 2))
    yield dict(obo=obo, gaf=gaf, folder=folder, loci=loci, keys=keys, gm=gm, ref=ref, xy=xy, parsed=parsed, table=table)
    gm.release()


def test_matrix_equals_the_restatement(case):
    gm, ref = case['gm'], case['ref']
    assert gm.loci == case['keys'] and gm.terms == ref['terms'] and gm.root == ref['root']
    assert np.array_equal(gm.missing_rows, ref['missing']) and gm.missing_rows.sum() == 2
    assert gm.num_root_assigned == ref['assigned'] and gm.num_root_assigned >= 3          # loci annotated in another branch only
    assert gm.matrix.format == 'csc' and gm.matrix.dtype == np.float32 and gm.matrix.shape == ref['ints'].shape
    assert gm.matrix.has_canonical_format and (gm.matrix.data == 1).all()
    assert np.array_equal(gm.matrix.toarray(), ref['ints'])
    assert np.array_equal(gm.matrix.toarray()[100], gm.matrix.toarray()[7])               # the key listed twice
    assert list(gm.go_details['id']) == gm.terms and list(gm.go_details['name'])[0].startswith('term ')
    assert set(gm.go_details['namespace']) == {'biological_process'}
    assert 1 < len(gm.terms) < N_TERMS                                                    # some term had no locus


def safe_on(amd, case):
    sf = amd.SAFE(verbose=False)
    sf.graph = amd.LayoutGraph(case['xy'], keys=case['keys'])
    sf.define_neighborhoods(node_distance_metric='euclidean', neighborhood_radius=0.1)
    return sf


@pytest.fixture(scope='module')
def dense_results(amd, case):
    sf = safe_on(amd, case)
    sf.load_attributes(attribute_file=case['ref']['dense'].copy())
    sf.compute_pvalues(how='hypergeometric')
    return np.array(sf.pvalues_pos), np.array(sf.nes)


@pytest.mark.parametrize('keep', [False, True])
def test_pvalues_bit_equal_to_the_dense_restatement(amd, case, dense_results, keep, monkeypatch):
    from safepy_amd import backend as be
    sf = safe_on(amd, case)
    expanded, uploaded = [], []
    real_expand, real_upload = be.GoClosure.as_attributes, be.Attributes.from_sparse.__func__
    monkeypatch.setattr(be.GoClosure, 'as_attributes', lambda self: expanded.append(1) or real_expand(self))
    monkeypatch.setattr(be.Attributes, 'from_sparse', classmethod(lambda cls, *a, **k: uploaded.append(1) or real_upload(cls, *a, **k)))
    assert case['gm'].on_device
    sf.load_attributes(attribute_file=case['gm'], keep_on_device=keep)
    assert (len(expanded), len(uploaded)) == ((1, 0) if keep else (0, 0))     # resident: expanded where the CSC lies, no upload
    assert sf.node2attribute is case['gm'].matrix
    assert sf.attributes['id'].tolist() == case['gm'].terms and sf.attributes['name'].tolist() == list(case['gm'].go_details['name'])
    assert (sf._resident_attributes() is not None) == keep
    sf.compute_pvalues(how='hypergeometric')
    assert (len(expanded), len(uploaded)) == ((1, 0) if keep else (0, len(uploaded))) and (keep or uploaded)   # not resident: the stored entries are uploaded
    p, nes = dense_results
    assert np.array_equal(np.array(sf.pvalues_pos).view(np.uint64), p.view(np.uint64))
    assert np.array_equal(np.array(sf.nes).view(np.uint64), nes.view(np.uint64))
    assert np.isfinite(p[~np.isnan(p)]).all() and (p[~np.isnan(p)] < 1).any()


def test_a_matrix_in_another_row_order_is_refused(amd, case):
    from safepy_amd.utils import make_go
    sf = safe_on(amd, case)
    plain = make_go.make_go_matrix(case['obo'], case['gaf'], 'p', write_files=False)        # rows: the file's sorted loci
    assert plain.loci == case['loci'] and plain.node_label_order is None
    with pytest.raises(ValueError, match='node_label_order'):
        sf.load_attributes(attribute_file=plain)
    plain.release()
    turned = make_go.make_go_matrix(case['obo'], case['gaf'], 'p', node_label_order=case['keys'][::-1], write_files=False)
    with pytest.raises(ValueError, match='node_label_order'):
        sf.load_attributes(attribute_file=turned, keep_on_device=True)
    turned.release()


def test_written_files(amd, case):
    import pandas as pd
    from safepy_amd.utils import make_go
    gm = make_go.make_go_matrix(case['obo'], case['gaf'], 'p')
    gm.release()
    ref = go_ref.matrix_ref(case['parsed'], list(zip(case['table'][1], case['table'][4])), 'p')
    assert gm.loci == case['loci'] == ref['loci'] and gm.terms == ref['terms'] and not gm.missing_rows.any()
    want = pd.DataFrame(ref['ints'].astype(int), index=ref['loci'], columns=ref['terms']).to_csv(sep='\t')
    with open(os.path.join(case['folder'], 'go_p_matrix.txt'), 'rb') as f:
        assert f.read() == want.encode('utf-8')
    with open(os.path.join(case['folder'], 'go_p.p'), 'rb') as f:
        saved = pickle.load(f)
    assert sorted(saved) == ['annotations_path', 'go_details', 'go_matrix', 'locus_details', 'tree_path']
    assert saved['tree_path'] == case['obo'] and saved['annotations_path'] == case['gaf']
    frame = saved['go_matrix']
    assert list(frame.index) == ref['loci'] and list(frame.columns) == ref['terms'] and np.array_equal(frame.to_numpy(), ref['ints'])
    assert all(isinstance(d, pd.SparseDtype) for d in frame.dtypes)
    assert len(saved['go_details']) == N_TERMS + 1 and len(saved['locus_details']) == len(case['table'])
    # the command line writes the same two files
    os.remove(os.path.join(case['folder'], 'go_p_matrix.txt'))
    make_go.main(['--path-to-obo', case['obo'], '--path-to-annotations', case['gaf'], '--go-branch', 'p'])
    with open(os.path.join(case['folder'], 'go_p_matrix.txt'), 'rb') as f:
        assert f.read() == want.encode('utf-8')
