"""Data preparation around SAFE (the counterpart of safepy/utils): make_go builds a gene-to-term attribute matrix from an
ontology file and an annotation file, with the propagation up the ontology done on the device."""
from .make_go import (GoGraph, GoMatrix, get_go_graph, make_go_matrix, make_locus2term, parse_go_obo,  # noqa: F401
                      read_annotations)
