"""Host side of pathpyg_amd.processes: the restatement of the walk contract (tests/cpu_ops_walks.py) held to forced walks, sinks, zero
weights, first-order sequences and one distribution check; the argument errors of RandomWalk, which are raised before any device work.  No
GPU is touched.  The distribution check runs on the restatement alone with a fixed seed: it is deterministic."""
import math

import pytest
import torch

import cpu_ops_walks as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip, _lib


def host_graph(edges, n, **attrs):
    """A row-sorted host Graph made without device work (num_nodes given, rows known to be sorted)."""
    ei = torch.tensor(sorted(edges), dtype=torch.int64).reshape(-1, 2).t().contiguous()
    return pp.Graph(pp.Data(edge_index=ei, num_nodes=n, **attrs), _row_sorted=True)


def csr(edges, n):
    edges = sorted(edges)
    row_ptr = [0] * (n + 1)
    for u, _ in edges:
        row_ptr[u + 1] += 1
    for v in range(n):
        row_ptr[v + 1] += row_ptr[v]
    return row_ptr, [v for _, v in edges]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("seed", [0, -1, 12345])
def test_cycle_forces_the_walk(seed):
    n = 7
    row_ptr, col = csr([(v, (v + 1) % n) for v in range(n)], n)
    got = ops.walks(row_ptr, col, None, seed, 20, [3, 0])
    assert got == [[(3 + t) % n for t in range(21)], [t % n for t in range(21)]]
    for how in ("weighted", "uniform"):
        for walk in ops.walks(row_ptr, col, None, seed, 9, how, num_walks=5):
            assert walk == [(walk[0] + t) % n for t in range(10)]


def test_sink_ends_walks():
    row_ptr, col = csr([(0, 1), (1, 2)], 4)                     # 2 and 3 are sinks, 3 is isolated
    assert ops.walks(row_ptr, col, None, 5, 10, [0, 1, 2, 3]) == [[0, 1, 2], [1, 2], [2], [3]]
    assert ops.padded([[0, 1, 2], [2]], 3) == ([[0, 1, 2, -1], [2, -1, -1, -1]], [2, 0])
    for how in ("weighted", "uniform"):                         # a drawn start is never a sink
        assert all(w[0] in (0, 1) for w in ops.walks(row_ptr, col, None, 5, 1, how, num_walks=200))


@pytest.mark.parametrize("zero_at", [0, 1, 2])
def test_zero_weight_entry_is_never_taken(zero_at):
    row_ptr, col = csr([(0, 1), (0, 2), (0, 3)], 4)
    weight = [1.0, 1.0, 1.0]
    weight[zero_at] = 0.0
    ends = {w[1] for w in ops.walks(row_ptr, col, weight, 3, 1, [0] * 2000)}
    assert ends == {1, 2, 3} - {1 + zero_at}
    row_ptr, col = csr([(0, 1), (1, 0)], 2)                     # a node whose only edge weighs 0 is a sink, and is never drawn as a start
    assert ops.walks(row_ptr, col, [0.0, 1.0], 3, 4, [0, 1]) == [[0], [1, 0]]
    assert all(w[0] == 1 for w in ops.walks(row_ptr, col, [0.0, 1.0], 3, 0, "weighted", num_walks=100))
    assert all(w[0] == 1 for w in ops.walks(row_ptr, col, [0.0, 1.0], 3, 0, "uniform", num_walks=100))


def test_first_order_of_a_second_order_walk():
    node_sequence = [[0, 1], [1, 2], [2, 0], [2, 3]]            # layer nodes of order 2
    assert ops.first_order([0, 1, 2, 0], node_sequence) == [0, 1, 2, 0, 1]          # k + length nodes
    assert ops.first_order([3], node_sequence) == [2, 3]
    fields = ops.path_data_fields([[0, 1, 3], [2], [1, 2]], node_sequence)
    assert fields["node_sequence"] == [[0], [1], [2], [3], [1], [2], [0]]
    assert fields["edge_index"] == [[0, 1, 2, 4, 5], [1, 2, 3, 5, 6]]
    assert fields["dag_num_nodes"] == [4, 3] and fields["dag_num_edges"] == [3, 2] and fields["dag_weight"] == [1.0, 1.0]


def test_start_tables():
    total = [0.0, 2.0, 0.0, 1.0] + [0.0] * 1020 + [4.0, 0.0]   # two blocks
    bcum, B = ops.start_table(total)
    assert bcum[:4] == [0.0, 2.0, 2.0, 3.0] and bcum[1023] == 3.0 and bcum[1024:] == [4.0, 4.0] and B == [3.0, 7.0]
    assert ops.positive_nodes(total) == [1, 3, 1024]
    draws = [ops.weighted_start(9, w, total, bcum, B) for w in range(700)]
    assert set(draws) == {1, 3, 1024}
    for node, p in ((1, 2 / 7), (3, 1 / 7), (1024, 4 / 7)):
        assert abs(draws.count(node) - 700 * p) <= 5 * math.sqrt(700 * p * (1 - p))


def test_transition_distribution():
    """2^16 one-step walks from a node with successors weighted 0.125 / 0.25 / 0.625: every count within 5 standard deviations of W p."""
    W = 1 << 16
    row_ptr, col = csr([(0, 1), (0, 2), (0, 3)], 4)
    p = [0.125, 0.25, 0.625]
    ends = [w[1] for w in ops.walks(row_ptr, col, p, 20240229, 1, [0] * W)]
    for node, q in zip((1, 2, 3), p):
        assert abs(ends.count(node) - W * q) <= 5 * math.sqrt(W * q * (1 - q)), (node, ends.count(node))


def test_restatement_refuses_bad_weights():
    row_ptr, col = csr([(0, 1)], 2)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.table(row_ptr, [bad])


# ------------------------------------------------------------------ the package: argument errors come before any device work
def test_argument_errors():
    g = host_graph([(0, 1), (1, 2), (2, 0)], 3, edge_weight=torch.ones(3))
    rw = pp.processes.RandomWalk(g, weight="edge_weight")
    with pytest.raises(ValueError):
        rw.run(num_walks=4, steps=-1)
    with pytest.raises(ValueError):
        rw.run(num_walks=4, steps=1.5)
    with pytest.raises(ValueError):
        rw.run(steps=3)                                         # neither num_walks nor explicit starts
    with pytest.raises(ValueError):
        rw.run(steps=3, start="uniform")
    with pytest.raises(ValueError):
        rw.run(num_walks=2, steps=3, start=torch.tensor([0, 1]))                    # both
    with pytest.raises(ValueError):
        rw.run(num_walks=2, steps=3, start=[0, 1])
    with pytest.raises(ValueError):
        rw.run(num_walks=-1, steps=3)
    with pytest.raises(ValueError):
        rw.run(num_walks=2, steps=3, start="somewhere")
    for bad in ([3], [-1], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            rw.run(steps=3, start=torch.tensor(bad))
        with pytest.raises(ValueError):
            rw.run(steps=3, start=bad)                          # (no ids in the mapping: a list holds indices)
    with pytest.raises(ValueError):
        rw.run(steps=3, start=torch.tensor([0.5]))
    with pytest.raises(AttributeError):                         # degrees()'s error for an unknown attribute ...
        pp.processes.RandomWalk(g, weight="edge_nothing")
    with pytest.raises(ValueError):                             # ... which is an argument error like the others
        pp.processes.RandomWalk(g, weight="edge_nothing")
    ids = pp.Graph(pp.Data(edge_index=torch.tensor([[0, 1], [1, 0]]), num_nodes=2), mapping=pp.IndexMap(["a", "b"]), _row_sorted=True)
    with pytest.raises(ValueError):
        pp.processes.RandomWalk(ids).run(steps=1, start=["a", "c"])


def test_size_refusals_are_arithmetic():
    """walks * (steps + order) must stay below 2^31 - 1, like n and m: refused from the arguments, nothing is allocated."""
    limit = (1 << 31) - 1
    _hip.walk_check_sizes(10, 10, 1 << 20, 2046, 1)             # 2^20 * 2047 = 2^31 - 2^20: allowed
    _hip.walk_check_sizes(10, 10, limit - 1, 0, 1)
    for args in ((10, 10, 1 << 20, 2047, 1), (10, 10, 1 << 20, 2046, 2), (10, 10, limit, 0, 1), (limit, 10, 1, 1, 1), (10, limit, 1, 1, 1),
                 (10, 10, 1, limit - 1, 1)):
        with pytest.raises(_lib.HipError, match="-4"):
            _hip.walk_check_sizes(*args)
    g = host_graph([(0, 1), (1, 0)], 2)
    with pytest.raises(_lib.HipError, match="-4"):
        pp.processes.RandomWalk(g).run(num_walks=1 << 20, steps=2047)
    model = pp.MultiOrderModel()
    with pytest.raises(ValueError):
        model.sample_walks(2, 10, 3)                            # no such layer


def test_seed_is_kept():
    assert hasattr(pp.processes, "last_seed")
    from pathpyg_amd.processes import random_walk
    assert random_walk._seed(-1) == (1 << 64) - 1 and pp.processes.last_seed == -1
    torch.manual_seed(7)
    a = random_walk._seed(None)
    torch.manual_seed(7)
    assert random_walk._seed(None) == a and pp.processes.last_seed & ((1 << 64) - 1) == a
