"""CPU suite: the user-graph builder's place in the C ABI, its argument checks (all of which return before any launch), the
GPU-only Python helper, and the rule itself — as independent nested loops — against the graphs and masks the reference minted."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from user_graph_common import RULE_FIXTURES, loop_rule, rule_fixture


def _lib_built():
    from digat_amd import _lib, build
    build.build(verbose=False)
    return _lib


def test_symbol_is_declared_and_exported():
    _lib = _lib_built()
    header = open(os.path.join(REPO, "include", "digat_hip.h")).read()
    assert "int digat_user_graph_build(" in header
    assert "digat_user_graph_build" in _lib.EXPORTED
    assert hasattr(_lib.lib(), "digat_user_graph_build")
    assert _lib.lib().digat_version() == 4          # a new symbol, the same ABI version


def test_argument_checks_return_before_any_launch():
    _lib = _lib_built()
    L = _lib.lib()
    dummy = ctypes.create_string_buffer(64)         # non-null host bytes: no path below dereferences or launches
    p = ctypes.addressof(dummy)
    ARG, SHAPE, OK = 1, 2, 0
    assert L.digat_user_graph_build(None, None, 1, 50, 17, p, p, None, None) == ARG
    assert L.digat_user_graph_build(p, None, 1, 50, 17, None, p, None, None) == ARG
    assert L.digat_user_graph_build(p, None, 1, 50, 17, p, None, None, None) == ARG
    assert L.digat_user_graph_build(p, None, -1, 50, 17, p, p, None, None) == ARG
    assert L.digat_user_graph_build(p, None, 1, -1, 17, p, p, None, None) == ARG
    assert L.digat_user_graph_build(p, None, 1, 100, 29, p, p, None, None) == SHAPE        # H + C = 129
    assert L.digat_user_graph_build(p, None, 1, 0, 17, p, p, None, None) == SHAPE
    assert L.digat_user_graph_build(p, None, 1, 50, 0, p, p, None, None) == SHAPE
    assert L.digat_user_graph_build(p, None, 0, 50, 17, p, p, None, None) == OK            # G == 0: nothing to do
    assert L.digat_user_graph_build(p, p, 0, 111, 17, p, p, p, None) == OK                 # ... at H + C = 128 too


def test_cpu_tensors_are_refused():
    from digat_amd import _lib, util
    with pytest.raises(_lib.DigatHipError):
        util.user_graphs_from_indices(torch.zeros((2, 10), dtype=torch.int64), 5)


@pytest.mark.parametrize("name", sorted(RULE_FIXTURES))
def test_loop_rule_reproduces_reference_minted_graphs(name):
    ci, C, graph, mask = rule_fixture(name)
    assert len(ci) >= 3
    got_graph, got_mask, entries = loop_rule(ci, C)
    assert np.array_equal(got_graph, graph) and np.array_equal(got_mask, mask)
    assert np.array_equal(entries, graph.reshape(len(graph), -1).sum(axis=1))
