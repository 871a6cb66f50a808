"""connected_components and largest_connected_component on the device (csrc/pp_graph_components.hip) through the public functions, held
to the fixtures made from scipy and the reference's own function (tests/golden/components_vectors.npz) and to the plain restatement
(tests/cpu_ops_components.py: sequential union-find and Tarjan, neither of which the kernels use), at the smallest shapes at which each
mechanism can fail: a hub whose edges all meet on one word, parent chains of thousands of nodes, sweep counts at their bound, several
rounds, labels ranked across many workgroups.  Everything is an integer and every comparison is exact."""
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_components as ops
import pathpyg_amd as pp
from pathpyg_amd import _dispatch
from pathpyg_amd.algorithms import connected_components, largest_connected_component

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "components_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]

REFERENCE_EXAMPLE = [("a", "b", 1), ("b", "c", 5), ("c", "d", 9), ("c", "e", 9), ("c", "f", 11), ("f", "a", 13), ("a", "g", 18), ("b", "f", 21),
                     ("a", "g", 26), ("c", "f", 27), ("h", "f", 27), ("g", "h", 28), ("a", "c", 30), ("a", "b", 31), ("c", "h", 32), ("f", "h", 33),
                     ("b", "i", 42), ("i", "b", 42), ("c", "i", 47), ("h", "i", 50)]


def graph_of(ei, n, device=DEV, ids=None, undirected=False):
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64).reshape(2, -1).to(device)
    mapping = None if ids is None else pp.IndexMap(list(ids))
    g = pp.Graph(pp.Data(edge_index=ei, num_nodes=n), mapping=mapping)
    g.is_undirected_flag = undirected
    return g


def check_labels(got, want):
    count, labels = got
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == want.shape
    assert count == (int(want.max()) + 1 if len(want) else 0)
    assert np.array_equal(labels, want)
    return labels


def host_expression(graph, labels):
    """What the issue pins largest_connected_component to, evaluated with this repository's own Graph.from_edge_list."""
    if len(labels) == 0:
        return pp.Graph.from_edge_list([], is_undirected=graph.is_undirected(), device=graph.device)
    x = ops.largest_label(labels)
    to_idx = graph.mapping.to_idx
    kept = [(v, w) for v, w in graph.edges if labels[to_idx(v)] == x and labels[to_idx(w)] == x]
    return pp.Graph.from_edge_list(kept, is_undirected=graph.is_undirected(), device=graph.device)


def ids_of(g):
    ids = g.mapping.node_ids
    return None if ids is None else np.asarray(ids).tolist()


def check_same_graph(got, want):
    assert got.n == want.n and ids_of(got) == ids_of(want)
    if ids_of(want) is not None:
        assert np.asarray(got.mapping.node_ids).dtype.kind == np.asarray(want.mapping.node_ids).dtype.kind
    assert got.data.edge_index.dtype == torch.int64 and torch.equal(got.data.edge_index.cpu(), want.data.edge_index.cpu())
    assert got.is_undirected() == want.is_undirected() and got.device == want.device
    assert got.edge_attrs() == [] and got.node_attrs() == []


def check_graph(g, lcc=True):
    """Both public functions on ``g`` against the restatement; returns the weak and strong labels."""
    ei, n = g.data.edge_index.cpu().numpy(), g.n
    out = []
    for connection in ("weak", "strong"):
        want = ops.labels(ei, n, strong=connection == "strong", undirected=g.is_undirected())
        out.append(check_labels(connected_components(g, connection), want))
        if lcc:
            check_same_graph(largest_connected_component(g, connection), host_expression(g, want))
    return out


# ------------------------------------------------------------------ 1. the fixtures
@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(name):
    get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
    ei, n = get("edge_index"), int(get("n"))
    ids = [f"v{i:03d}" for i in range(n)]
    g = graph_of(ei, n, ids=ids)
    check_labels(connected_components(g), get("weak"))                                  # scipy's array itself
    count, strong = connected_components(g, "strong")
    assert count == int(get("strong").max()) + 1 and np.array_equal(strong, ops.by_smallest_member(get("strong")))
    flagged = graph_of(ei, n, ids=ids, undirected=True)
    for connection in ("weak", "strong"):
        check_labels(connected_components(flagged, connection), get("undirected"))
    for kind, graph, connection in (("weak", g, "weak"), ("strong", g, "strong"), ("undirected", flagged, "strong")):
        kept = get(f"lcc_{kind}")
        want = pp.Graph.from_edge_list([(ids[u], ids[w]) for u, w in kept.T.tolist()], is_undirected=graph.is_undirected(), device=DEV)
        check_same_graph(largest_connected_component(graph, connection), want)


# ------------------------------------------------------------------ 2. degenerate graphs
def test_no_nodes():
    g = graph_of(np.zeros((2, 0), dtype=np.int64), 0)
    for connection in ("weak", "strong"):
        count, labels = connected_components(g, connection)
        assert count == 0 and labels.dtype == np.int32 and labels.shape == (0,)
        lcc = largest_connected_component(g, connection)
        assert lcc.n == 0 and lcc.data.edge_index.shape == (2, 0) and lcc.device == g.device


def test_no_edges():
    g = graph_of(np.zeros((2, 0), dtype=np.int64), 5)
    for connection in ("weak", "strong"):
        check_labels(connected_components(g, connection), np.arange(5, dtype=np.int32))
        assert largest_connected_component(g, connection).n == 0


def test_one_node_with_a_self_loop():
    g = graph_of([[0], [0]], 1, ids=["only"])
    for connection in ("weak", "strong"):
        check_labels(connected_components(g, connection), np.zeros(1, dtype=np.int32))
        lcc = largest_connected_component(g, connection)
        assert lcc.n == 1 and ids_of(lcc) == ["only"] and lcc.data.edge_index.cpu().tolist() == [[0], [0]]
        check_same_graph(lcc, host_expression(g, np.zeros(1, dtype=np.int32)))


def test_largest_component_is_one_node_without_a_loop():
    g = graph_of([[1], [2]], 3, ids=["x", "y", "z"])
    check_labels(connected_components(g, "strong"), np.arange(3, dtype=np.int32))
    lcc = largest_connected_component(g, "strong")                              # three singletons: x is taken, and no edge names it
    assert lcc.n == 0 and lcc.data.edge_index.shape == (2, 0) and ids_of(lcc) is None
    check_same_graph(lcc, host_expression(g, np.arange(3, dtype=np.int32)))


# ------------------------------------------------------------------ 3. a hub: one contended word, a row above one wave and one workgroup
LEAVES = 5000


def star(hub_last: bool, towards_hub: bool) -> np.ndarray:
    hub = LEAVES if hub_last else 0
    leaves = np.arange(LEAVES) if hub_last else np.arange(1, LEAVES + 1)
    pair = (leaves, np.full(LEAVES, hub)) if towards_hub else (np.full(LEAVES, hub), leaves)
    return np.stack(pair).astype(np.int64)


@pytest.mark.parametrize("hub_last", [True, False])
@pytest.mark.parametrize("towards_hub", [True, False])
def test_star_hub(hub_last, towards_hub):
    n = LEAVES + 1
    g = graph_of(star(hub_last, towards_hub), n)
    check_labels(connected_components(g, "weak"), np.zeros(n, dtype=np.int32))
    check_labels(connected_components(g, "strong"), np.arange(n, dtype=np.int32))
    lcc = largest_connected_component(g)
    assert lcc.n == n and lcc.data.edge_index.size(1) == LEAVES
    check_same_graph(lcc, host_expression(g, np.zeros(n, dtype=np.int32)))


# ------------------------------------------------------------------ 4. long chains
def permuted(ei, n, seed):
    perm = np.random.default_rng(seed).permutation(n)
    return perm[np.asarray(ei)]


def strong_stats(g):
    return _dispatch.graph_components(g, True, with_stats=True)[3]


def test_undirected_path_of_20000_permuted_nodes():
    n = 20_000
    step = np.stack([np.arange(n - 1), np.arange(1, n)])
    g = graph_of(permuted(np.concatenate([step, step[::-1]], axis=1), n, 1), n, undirected=True)
    for connection in ("weak", "strong"):
        check_labels(connected_components(g, connection), np.zeros(n, dtype=np.int32))
    one_way = graph_of(permuted(step, n, 2), n)                                 # half the edges: the weak components of a directed path
    check_labels(connected_components(one_way), np.zeros(n, dtype=np.int32))


def test_directed_path_is_finished_by_trimming_alone():
    n = 3000
    g = graph_of(permuted(np.stack([np.arange(n - 1), np.arange(1, n)]), n, 3), n)
    check_labels(connected_components(g, "strong"), np.arange(n, dtype=np.int32))
    rounds, trim, colour, back = strong_stats(g)
    assert rounds == 0 and colour <= 1 and back == 0 and 1 <= trim <= n + 1     # (a sweep may see the removals of its own launch: no lower bound)


def test_directed_ring_needs_thousands_of_sweeps():
    n = 3000
    ring = permuted(np.stack([np.arange(n), (np.arange(n) + 1) % n]), n, 4)
    g = graph_of(ring, n)
    check_labels(connected_components(g, "strong"), np.zeros(n, dtype=np.int32))
    check_labels(connected_components(g, "weak"), np.zeros(n, dtype=np.int32))
    rounds, trim, colour, back = strong_stats(g)
    assert rounds == 1 and 1 <= trim <= n + 1 and 1 <= colour <= n + 1 and 1 <= back <= n + 1


# ------------------------------------------------------------------ 5. more than one round
@pytest.mark.parametrize("ascending", [False, True])
def test_chain_of_rings_takes_rounds(ascending):
    rings, k = 6, 5
    n = rings * k
    name = (lambda r, i: r * k + i) if ascending else (lambda r, i: n - 1 - (r * k + i))
    edges = [(name(r, i), name(r, (i + 1) % k)) for r in range(rings) for i in range(k)]
    edges += [(name(r, 0), name(r + 1, 0)) for r in range(rings - 1)]
    g = graph_of(np.array(edges).T, n)
    weak, strong = check_graph(g)
    assert weak.max() == 0 and strong.max() == rings - 1
    rounds = strong_stats(g)[0]
    assert 1 <= rounds <= rings
    if not ascending:                                                           # the largest index sits in the FIRST ring and colours them all
        assert rounds >= 2


def test_two_rings_a_tail_and_an_isolated_node():
    k = 50
    edges = [(i, (i + 1) % k) for i in range(k)] + [(k + i, k + (i + 1) % k) for i in range(k)]
    edges += [(7, k + 3), (k + 9, 100), (100, 101)]                             # ring -> ring, then a two-edge tail; node 102 is alone
    g = graph_of(np.array(edges).T, 103)
    weak, strong = check_graph(g)
    assert weak.max() + 1 == 2 and strong.max() + 1 == 5


# ------------------------------------------------------------------ 6. labels ranked across workgroups
def test_triangles_and_isolated_nodes_across_workgroups():
    triangles, alone = 4096, 1000
    n = 3 * triangles + alone
    base = 3 * np.arange(triangles)
    ei = np.concatenate([np.stack([base, base + 1]), np.stack([base + 1, base + 2]), np.stack([base + 2, base])], axis=1)
    perm = np.random.default_rng(6).permutation(n)
    g = graph_of(perm[ei], n)
    for connection in ("weak", "strong"):
        want = ops.labels(perm[ei], n, strong=connection == "strong")
        labels = check_labels(connected_components(g, connection), want)
        assert labels.max() + 1 == triangles + alone
        assert (labels[perm[base]] == labels[perm[base + 1]]).all() and (labels[perm[base]] == labels[perm[base + 2]]).all()
        count, dev_labels, sizes = _dispatch.graph_components(g, connection == "strong")
        assert int(count.item()) == triangles + alone
        assert np.array_equal(sizes.cpu().numpy()[:triangles + alone], ops.sizes(want)) and int(sizes[triangles + alone:].sum()) == 0
        assert np.array_equal(dev_labels.cpu().numpy(), want)


# ------------------------------------------------------------------ 7. determinism
def test_results_are_identical_from_run_to_run():
    big = NAMES[-1]
    graphs = [graph_of(GOLDEN[f"{big}/edge_index"], int(GOLDEN[f"{big}/n"])), graph_of(star(True, True), LEAVES + 1)]
    for g in graphs:
        for connection in ("weak", "strong"):
            first, second = connected_components(g, connection), connected_components(g, connection)
            assert first[0] == second[0] and np.array_equal(first[1], second[1])
            a, b = largest_connected_component(g, connection), largest_connected_component(g, connection)
            check_same_graph(a, b)


# ------------------------------------------------------------------ 8. staging and containers
def test_host_resident_graph_equals_its_device_copy():
    rng = np.random.default_rng(8)
    ei = rng.integers(0, 80, (2, 120))
    ids = [f"n{i}" for i in range(80)]
    host, dev = graph_of(ei, 80, device="cpu", ids=ids), graph_of(ei, 80, ids=ids)
    for connection in ("weak", "strong"):
        a, b = connected_components(host, connection), connected_components(dev, connection)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
        on_host = largest_connected_component(host, connection)
        assert on_host.device == torch.device("cpu")
        on_dev = largest_connected_component(dev, connection)
        assert ids_of(on_host) == ids_of(on_dev) and torch.equal(on_host.data.edge_index, on_dev.data.edge_index.cpu())
    check_graph(host)


def test_rolling_window_and_aggregate():
    t = pp.TemporalGraph.from_edge_list(REFERENCE_EXAMPLE, device=DEV)
    windows = list(pp.algorithms.RollingTimeWindow(t, 10, 10))
    assert len(windows) >= 3
    for g in windows:
        check_graph(g)
    weak, strong = check_graph(t.to_static_graph())
    assert weak.max() == 0 and strong.max() > 0


def test_second_order_layer_with_tuple_ids():
    t = pp.TemporalGraph.from_edge_list(REFERENCE_EXAMPLE, device=DEV)
    layer = pp.MultiOrderModel.from_temporal_graph(t, delta=15, max_order=2).layers[2]
    assert layer.order == 2 and layer.n > 2
    weak, strong = check_graph(layer, lcc=False)
    for connection, labels in (("weak", weak), ("strong", strong)):            # tuple IDs: the host expression itself, whatever it does with them
        try:
            want = host_expression(layer, labels)
        except Exception as error:  # noqa: BLE001 - the same failure is then expected of the function
            with pytest.raises(type(error)):
                largest_connected_component(layer, connection)
        else:
            check_same_graph(largest_connected_component(layer, connection), want)


# ------------------------------------------------------------------ 9. the sub-graph
@pytest.mark.parametrize("ids", [["10", "9", "2", "b", "30"], ["10", "9", "2", "100", "30"], None, [5, 3, 11, 7, 2]])
def test_lcc_orders_ids_as_from_edge_list_does(ids):
    ei = np.array([[3, 0, 1, 0, 3], [0, 1, 3, 0, 1]])                           # nodes 0, 1, 3 are one component; 2 and 4 are alone
    g = graph_of(ei, 5, ids=ids)
    weak, strong = check_graph(g)
    lcc = largest_connected_component(g)
    assert lcc.n == 3 and lcc.data.edge_index.size(1) == 5
    if ids == ["10", "9", "2", "b", "30"]:
        assert ids_of(lcc) == ["10", "9", "b"]                                  # as strings
    if ids == ["10", "9", "2", "100", "30"]:
        assert ids_of(lcc) == ["9", "10", "100"]                                # all numeric: as numbers
    if ids is None:
        assert ids_of(lcc) == [0, 1, 3]


def test_equal_largest_sizes_take_the_smaller_first_node():
    ei = np.array([[4, 5, 1, 2, 6], [5, 4, 2, 1, 6]])                           # {1, 2} and {4, 5}: both of size 2; 0, 3, 6 alone
    g = graph_of(ei, 7, ids=list("abcdefg"))
    check_graph(g)
    for connection in ("weak", "strong"):
        assert sorted(largest_connected_component(g, connection).nodes) == ["b", "c"]


def test_strong_giant_is_smaller_than_the_weak_one():
    edges = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 6), (7, 8), (8, 7)]
    g = graph_of(np.array(edges).T, 9, ids=[f"s{i}" for i in range(9)])
    check_graph(g)
    assert largest_connected_component(g, "weak").n == 7 and largest_connected_component(g, "strong").n == 3
    assert largest_connected_component(g, "STRONG").nodes == ["s0", "s1", "s2"]


def test_undirected_graph_keeps_its_flag():
    g = pp.Graph.from_edge_list([("a", "b"), ("b", "c"), ("d", "e")], device=DEV).to_undirected()
    assert g.is_undirected()
    check_graph(g)
    for connection in ("weak", "strong"):
        lcc = largest_connected_component(g, connection)
        assert lcc.is_undirected() and lcc.nodes == ["a", "b", "c"] and lcc.data.edge_index.size(1) == 4
    one_way = pp.Graph.from_edge_list([("a", "b"), ("b", "c"), ("d", "e")], is_undirected=True, device=DEV)      # flagged, one direction stored
    count, labels = connected_components(one_way, "strong")
    assert count == 2 and labels.tolist() == [0, 0, 0, 1, 1]
