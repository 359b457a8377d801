"""Shared by test_user_graph_cpu.py and test_hip_user_graph.py: the user-graph rule as plain nested loops (the yardstick the
kernel is held to, itself held to reference-minted fixtures by the CPU suite), and the fixtures that carry such graphs."""
import numpy as np

from conftest import load_golden

# fixture -> number of leading rows that follow the rule (row 5 of edges.npz is a deliberately irregular graph)
RULE_FIXTURES = {"tiny.npz": None, "train_step.npz": None, "train_step_dropout.npz": None, "ablation_wo_interaction_tiny.npz": None,
                 "edges.npz": 5}


def loop_rule(cat_idx, C):
    """(graph [G,U,U] bool, mask [G,C+1] bool, entries [G]) of category indices [G,H], one element at a time."""
    cat_idx = np.asarray(cat_idx)
    G, H = cat_idx.shape
    U = H + C
    graph = np.zeros((G, U, U), dtype=bool)
    mask = np.zeros((G, C + 1), dtype=bool)
    for g in range(G):
        idx = [int(v) for v in cat_idx[g]]
        valid = [0 <= v < C for v in idx]
        present = [any(valid[t] and idx[t] == c for t in range(H)) for c in range(C)]
        for i in range(H):
            for j in range(H):
                graph[g, i, j] = i == j or (valid[i] and valid[j] and idx[i] == idx[j])
            for c in range(C):
                graph[g, i, H + c] = graph[g, H + c, i] = valid[i] and idx[i] == c
        for a in range(C):
            for b in range(C):
                graph[g, H + a, H + b] = a == b or (present[a] and present[b])
            mask[g, a] = present[a]
    return graph, mask, graph.reshape(G, -1).sum(axis=1)


def rule_fixture(name):
    """(category indices, C, golden graph, golden mask) of the rows of fixture ``name`` that follow the rule."""
    fx = load_golden(name)
    n = RULE_FIXTURES[name]
    ci, g, m = (fx[k][:n] for k in ("in_user_category_indices", "in_user_graph", "in_user_category_mask"))
    return ci, m.shape[1] - 1, g, m


def scattered_indices(rng, rows, H, C):
    """Category indices whose valid slots do NOT form a prefix: valid and padding slots interleaved, a few negative and
    too-large values among them."""
    idx = rng.integers(0, C, size=(rows, H)).astype(np.int64)
    idx[rng.random((rows, H)) < 0.4] = C
    idx[rng.random((rows, H)) < 0.05] = -1
    idx[rng.random((rows, H)) < 0.05] = C + 3
    if rows > 1:
        idx[1] = C                         # a user without any valid slot
    return idx
