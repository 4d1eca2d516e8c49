"""The Kamada-Kawai entry points are declared, bound and exported, and the parts of the Python layer that need no device
behave as networkx's do."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('safe_kk_create_host', 'safe_kk_create_nbr', 'safe_kk_eval', 'safe_kk_destroy')


def test_kk_symbols_are_declared_bound_and_exported():
    from safepy_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'safe_hip.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), name
    assert int(re.search(r'#define SAFE_KK_MAX_NODES (\d+)', header).group(1)) == _lib.KK_MAX_NODES
    # every declaration cites the reference code it replaces and networkx's functions
    doc = header[header.index('Kamada-Kawai layout:'):header.index('int safe_kk_destroy')]
    assert doc.count('safe_io.py:288-308') >= 4
    for fn in ('kamada_kawai_layout', '_kamada_kawai_solve', '_kamada_kawai_costfn'):
        assert fn in doc, fn


def test_empty_graph_and_argument_checks_need_no_device():
    import networkx as nx
    import safepy_amd
    from safepy_amd import safe_io
    assert safe_io.kamada_kawai_layout(nx.Graph()) == {}
    G = safepy_amd.LayoutGraph(np.zeros((0, 2)))
    assert safe_io.kamada_kawai_layout(G) is G and G.xy.shape == (0, 2)
    with pytest.raises(ValueError, match='center'):
        safe_io.kamada_kawai_layout(nx.path_graph(3), center=(0, 0, 0))
    with pytest.raises(NotImplementedError):
        safe_io.kamada_kawai_layout(nx.DiGraph([(0, 1)]))


def test_apply_network_layout_names_the_layout_function():
    import networkx as nx
    from safepy_amd import safe_io
    with pytest.raises(NotImplementedError, match=r'safe_io\.kamada_kawai_layout.*spring_embedded'):
        safe_io.apply_network_layout(nx.path_graph(3), layout='kamada_kawai', verbose=False)
    assert 'later change' in safe_io.apply_network_layout.__doc__
