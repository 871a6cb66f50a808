"""Static shortest paths, closeness and betweenness on the device (csrc/pp_graph_paths.hip) through the public functions, held to the
fixtures made from the reference's own function, scipy and networkx (tests/golden/static_paths_vectors.npz) and to the plain restatement
(tests/cpu_ops_static_paths.py), at the smallest shapes at which each mechanism can fail: many levels with a frontier of one, a hub row
far above one wave and a frontier above one workgroup, more sources than workgroups, no edges at all.

dist, pred, diameter, avg_path_length, closeness and the betweenness key sets are exact.  Betweenness values: 1e-10 relative, 1e-10
absolute at zero — all terms are non-negative, so another summation order moves a sum by at most (number of additions) * 2^-53 relative,
and no sum here has more than 10^6 terms (the star's hub sums 5000 terms 5001 times; its value is an integer below 2^53 and exact)."""
import math
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_static_paths as ops
import pathpyg_amd as pp
from pathpyg_amd import _dispatch, _hip
from pathpyg_amd.algorithms import centrality as ct
from pathpyg_amd.algorithms import shortest_paths as sp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "static_paths_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]
TOL = dict(rtol=1e-10, atol=1e-10)

REFERENCE_EXAMPLE = [("a", "b", 1), ("b", "c", 5), ("c", "d", 9), ("c", "e", 9), ("c", "f", 11), ("f", "a", 13), ("a", "g", 18), ("b", "f", 21),
                     ("a", "g", 26), ("c", "f", 27), ("h", "f", 27), ("g", "h", 28), ("a", "c", 30), ("a", "b", 31), ("c", "h", 32), ("f", "h", 33),
                     ("b", "i", 42), ("i", "b", 42), ("c", "i", 47), ("h", "i", 50)]


def graph_of(ei, n, device=DEV, ids=None):
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64).reshape(2, -1).to(device)
    mapping = None if ids is None else pp.IndexMap(list(ids))
    return pp.Graph(pp.Data(edge_index=ei, num_nodes=n), mapping=mapping)


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_pred_valid(dist, pred, ei, n):
    off = ~np.eye(n, dtype=bool)
    rows, cols = np.nonzero(np.isfinite(dist) & off)
    p = pred[rows, cols].astype(np.int64)
    assert ((p >= 0) & (p < n)).all()
    assert (dist[rows, p] + 1 == dist[rows, cols]).all()
    ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
    assert np.isin(p * n + cols, ei[0] * n + ei[1]).all()                 # (pred[i, j], j) is a stored edge
    assert (pred[~(np.isfinite(dist) & off)] == -9999).all()


def check_graph(g, ei, n, want=None, ids=None):
    """Every public function on ``g`` against the restatement on the edge list."""
    want = ops.all_sources(ei, n) if want is None else want
    ids = list(range(n)) if ids is None else ids
    dist, pred = sp.shortest_paths_dijkstra(g)
    assert dist.dtype == np.float64 and pred.dtype == np.int32 and dist.shape == pred.shape == (n, n)
    assert np.array_equal(dist, want["dist"])
    check_pred_valid(dist, pred, ei, n)
    assert np.array_equal(pred, want["pred"])                             # the largest tight predecessor index
    assert same_float(sp.diameter(g), ops.diameter(want["dist"]))
    assert same_float(sp.avg_path_length(g), ops.avg_path_length(want["dist"]))
    cl = ct.closeness_centrality(g)
    assert list(cl) == ids and list(cl.values()) == ops.closeness(want["dist"]).tolist()
    bw = ct.betweenness_centrality(g)
    assert set(bw) == {ids[i] for i in np.nonzero(want["keys"])[0]}
    np.testing.assert_allclose([bw[ids[i]] if ids[i] in bw else 0.0 for i in range(n)], want["bw"], **TOL)
    return dist, pred, cl, bw


@pytest.mark.parametrize("name", NAMES)
def test_fixture_case(name):
    get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
    ei, n = get("edge_index"), int(get("n"))
    ids = [f"v{i:03d}" for i in range(n)]
    g = graph_of(ei, n, ids=ids)
    dist, _, cl, bw = check_graph(g, ei, n, ids=ids)
    gold = get("dist").astype(np.float64)
    gold[gold < 0] = np.inf
    assert np.array_equal(dist, gold)
    assert list(cl.values()) == get("closeness").tolist()
    assert set(bw) == {ids[i] for i in np.nonzero(get("bw_keys"))[0]}
    np.testing.assert_allclose([bw[i] if i in bw else 0.0 for i in ids], get("bw"), **TOL)
    assert bw["no such node"] == 0.0                                      # a defaultdict, as the reference returns
    sub = ct.betweenness_centrality(g, sources=[ids[s] for s in get("sources")])          # one id twice: it counts twice
    assert set(sub) == {ids[i] for i in np.nonzero(get("sub_bw_keys"))[0]}
    np.testing.assert_allclose([sub[i] if i in sub else 0.0 for i in ids], get("sub_bw"), **TOL)


def test_reference_known_answers():
    tri = pp.Graph.from_edge_list([("a", "b"), ("b", "a"), ("b", "c"), ("c", "b"), ("a", "c"), ("c", "a")], is_undirected=True, device=DEV)
    assert dict(ct.betweenness_centrality(tri)) == {"a": 0.0, "b": 0.0, "c": 0.0}
    assert ct.closeness_centrality(tri) == {"a": 1.0, "b": 1.0, "c": 1.0}
    g = pp.Graph.from_edge_list([("a", "b"), ("b", "c"), ("c", "e"), ("b", "d"), ("d", "e")], device=DEV).to_undirected()
    dist, pred = sp.shortest_paths_dijkstra(g)
    assert np.array_equal(dist, np.array([[0, 1, 2, 2, 3], [1, 0, 1, 1, 2], [2, 1, 0, 2, 1], [2, 1, 2, 0, 1], [3, 2, 1, 1, 0]], dtype=np.float64))
    for i in range(5):
        for j in range(5):
            if i != j:
                assert dist[i, j] == dist[i, pred[i, j]] + 1
    assert pp.algorithms.shortest_paths.diameter(g) == 3 and pp.algorithms.shortest_paths.avg_path_length(g) == 1.6


@pytest.mark.parametrize("n", [1, 5])
def test_no_edges(n):
    g = graph_of(np.zeros((2, 0), dtype=np.int64), n)
    dist, pred = sp.shortest_paths_dijkstra(g)
    assert (pred == -9999).all() and pred.shape == (n, n)
    assert (np.diag(dist) == 0).all() and np.isinf(dist[~np.eye(n, dtype=bool)]).all()
    assert dict(ct.betweenness_centrality(g)) == {}
    assert ct.closeness_centrality(g) == {i: 0.0 for i in range(n)}
    assert sp.diameter(g) == (0.0 if n == 1 else math.inf)
    assert math.isnan(sp.avg_path_length(g)) if n == 1 else sp.avg_path_length(g) == math.inf


def test_directed_path_many_levels_with_a_frontier_of_one():
    n = 300
    ei = np.stack([np.arange(n - 1), np.arange(1, n)])
    dist, pred, _, bw = check_graph(graph_of(ei, n), ei, n)
    assert dist[0, n - 1] == n - 1 and pred[0, n - 1] == n - 2 and np.isinf(dist[n - 1, 0])
    assert bw[1] == float(n - 2) and bw[n - 1] == 0.0 and 0 not in bw   # node k collects (k sources) * (n - 1 - k dependants)


LEAVES = 5000


def star(kind):
    hub, leaves = np.zeros(LEAVES, dtype=np.int64), np.arange(1, LEAVES + 1)
    out, into = np.stack([hub, leaves]), np.stack([leaves, hub])
    return {"out": out, "in": into, "both": np.concatenate([out, into], axis=1)}[kind]


@pytest.mark.parametrize("kind", ["out", "in", "both"])
def test_star_hub_row_far_above_one_wave(kind):
    n = LEAVES + 1
    ei = star(kind)
    g = graph_of(ei, n)
    picks = [0, 1, 77, LEAVES]
    dist, pred = (t.cpu().numpy() for t in _dispatch.graph_shortest_paths(g, picks))          # four rows of the dense result
    want_dist, want_pred = ops.shortest_paths(ei, n, picks)
    assert np.array_equal(np.where(dist >= 0, dist, np.inf), want_dist) and np.array_equal(pred, want_pred)
    bw, cl = ct.betweenness_centrality(g), ct.closeness_centrality(g)
    leaves = range(1, n)
    if kind == "out":                   # the hub reaches every leaf at distance 1; nothing else is reachable
        assert set(bw) == set(leaves) and not any(bw.values())
        assert cl[0] == 0.0 and all(cl[v] == (1 / 1) * (1 / LEAVES) for v in leaves)
        assert sp.diameter(g) == math.inf and sp.avg_path_length(g) == math.inf
    elif kind == "in":                  # every leaf reaches the hub, the hub is the last level of every search
        assert dict(bw) == {0: 0.0}
        assert cl[0] == 1.0 and not any(cl[v] for v in leaves)
        assert sp.diameter(g) == math.inf
    else:                               # a leaf's search: the hub (npred 1) sums 4999 dependants; the hub's own search adds nothing
        assert set(bw) == set(range(n)) and bw[0] == float(LEAVES * (LEAVES - 1)) and not any(bw[v] for v in leaves)
        assert cl[0] == 1.0 and all(cl[v] == (LEAVES / (2 * LEAVES - 1)) * (LEAVES / LEAVES) for v in leaves)
        assert sp.diameter(g) == 2.0
        assert sp.avg_path_length(g) == float(np.float64(2 * LEAVES + 2 * LEAVES * (LEAVES - 1)) / (n * (n - 1)))


def test_small_star_and_hubs_against_the_restatement():
    # 200 leaves on an undirected hub plus a second hub with 70 parallel edges and a self-loop: rows of 64 entries and more, all outputs
    hub, leaves = np.zeros(200, dtype=np.int64), np.arange(1, 201)
    extra = np.stack([np.full(71, 201), np.r_[np.full(70, 5), 201]])
    ei = np.concatenate([np.stack([hub, leaves]), np.stack([leaves, hub]), extra, np.array([[7], [201]])], axis=1)
    check_graph(graph_of(ei, 202), ei, 202)


N_BIG, M_BIG = 2500, 7500


@pytest.fixture(scope="module")
def big():
    """Seeded sparse random digraph with more sources than either kernel has workgroups, and its restatement (computed once)."""
    ei = np.random.default_rng(2500).integers(0, N_BIG, (2, M_BIG))
    ei = ei[:, np.argsort(ei[0], kind="stable")]
    return ei, ops.all_sources(ei, N_BIG), graph_of(ei, N_BIG)


def test_more_sources_than_workgroups(big):
    ei, want, g = big
    L = _hip.lib()
    assert L.pp_graph_bfs_parts(N_BIG, N_BIG) == 2048 and L.pp_graph_betweenness_parts(N_BIG, N_BIG) == 1024
    assert L.pp_graph_bfs_ws_bytes(N_BIG, N_BIG) >= 2048 * 2 * N_BIG * 4
    check_graph(g, ei, N_BIG, want=want)


def test_scalars_survive_the_later_sources_of_a_workgroup():
    """An undirected path of 3000 nodes whose two END nodes carry the indices 0 and 1: strongly connected (every total is finite) with more
    sources than workgroups, and the largest eccentricities belong to the FIRST sources of workgroups 0 and 1, which finish with interior
    nodes.  The longest distance and the sum of distances have to outlive every later source of the same workgroup.  The expected distance
    matrix is |position - position|; the restatement's search confirms rows of it, its totals give diameter, average and closeness."""
    n = 3000
    chain = np.r_[0, np.arange(2, n), 1]                                  # the node at every position of the path
    pos = np.empty(n, dtype=np.int64)
    pos[chain] = np.arange(n)
    a, b = chain[:-1], chain[1:]
    ei = np.concatenate([np.stack([a, b]), np.stack([b, a])], axis=1)
    want = np.abs(pos[:, None] - pos[None, :]).astype(np.float64)
    picks = [0, 1, 2, 2048, 2049, n - 1]
    rows, _ = ops.shortest_paths(ei, n, picks)
    assert np.array_equal(rows, want[picks])
    L = _hip.lib()
    assert L.pp_graph_bfs_parts(n, n) == 2048 and L.pp_graph_betweenness_parts(n, n) == 1024
    g = graph_of(ei, n)
    assert sp.diameter(g) == ops.diameter(want) == float(n - 1)
    assert sp.avg_path_length(g) == ops.avg_path_length(want)
    assert list(ct.closeness_centrality(g).values()) == ops.closeness(want).tolist()
    dist, pred = sp.shortest_paths_dijkstra(g)
    assert np.array_equal(dist, want)
    check_pred_valid(dist, pred, ei, n)
    bw = ct.betweenness_centrality(g)                                     # every source left of a node meets every node right of it, and back
    assert set(bw) == set(range(n))
    np.testing.assert_allclose([bw[v] for v in range(n)], 2.0 * pos * (n - 1 - pos), **TOL)


def test_totals_route_builds_nothing_dense(big, monkeypatch):
    ei, want, g = big

    def refuse(*a, **k):
        raise AssertionError("the dense search was called on the totals-only route")
    monkeypatch.setattr(_hip, "graph_bfs_dense", refuse)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert same_float(sp.diameter(g), ops.diameter(want["dist"]))
    assert same_float(sp.avg_path_length(g), ops.avg_path_length(want["dist"]))
    assert list(ct.closeness_centrality(g).values()) == ops.closeness(want["dist"]).tolist()
    # the 2048 workgroup slices of 2 * n int32 plus O(n) sources, totals and staging; ONE n x n int32 matrix would add 25 MB, so half of
    # that separates the two without depending on the allocator's rounding of the small pieces
    assert torch.cuda.max_memory_allocated() - before < SLICE_BYTES + N_BIG * N_BIG * 4 // 2
    with pytest.raises(AssertionError):
        sp.shortest_paths_dijkstra(g)


SLICE_BYTES = 2048 * 2 * N_BIG * 4


def test_betweenness_is_bit_identical_from_run_to_run(big):
    _, _, g = big
    first, second = ct.betweenness_centrality(g), ct.betweenness_centrality(g)
    assert list(first.items()) == list(second.items())


def test_host_resident_graph_equals_its_device_copy():
    rng = np.random.default_rng(3)
    ei = rng.integers(0, 60, (2, 200))
    host = graph_of(ei, 60, device="cpu")
    dist_h, pred_h = sp.shortest_paths_dijkstra(host)
    rest_h = (sp.diameter(host), sp.avg_path_length(host), ct.closeness_centrality(host), dict(ct.betweenness_centrality(host)),
              dict(ct.betweenness_centrality(host, sources=[3, 59, 3])))
    assert host.data.edge_index.device.type == "cpu"
    dev = host.to(DEV)
    assert dev.data.edge_index.is_cuda
    dist_d, pred_d = sp.shortest_paths_dijkstra(dev)
    assert np.array_equal(dist_h, dist_d) and np.array_equal(pred_h, pred_d)
    assert rest_h == (sp.diameter(dev), sp.avg_path_length(dev), ct.closeness_centrality(dev), dict(ct.betweenness_centrality(dev)),
                      dict(ct.betweenness_centrality(dev, sources=[3, 59, 3])))
    check_graph(dev, dev.data.edge_index.cpu().numpy(), 60)


def test_sources_out_of_range_or_unknown_raise():
    g = pp.Graph.from_edge_list([("a", "b"), ("b", "c")], device=DEV)
    with pytest.raises(KeyError):
        ct.betweenness_centrality(g, sources=["a", "nobody"])
    plain = graph_of([[0, 1], [1, 2]], 3)
    with pytest.raises(IndexError):
        ct.betweenness_centrality(plain, sources=[0, 3])


def test_second_order_layer_with_tuple_ids():
    t = pp.TemporalGraph.from_edge_list(REFERENCE_EXAMPLE, device=DEV)
    layer = pp.MultiOrderModel.from_temporal_graph(t, delta=15, max_order=2).layers[2]
    n = layer.n
    ei = layer.data.edge_index.cpu().numpy()
    assert n > 2 and ei.shape[1] > 2
    ids = [layer.mapping.to_id(i) for i in range(n)]
    assert all(isinstance(i, tuple) and len(i) == 2 for i in ids)
    _, _, cl, bw = check_graph(layer, ei, n, ids=ids)
    assert any(v > 0 for v in bw.values()) and any(v > 0 for v in cl.values())
    some = [ids[0], ids[n - 1], ids[0]]
    sub = ct.betweenness_centrality(layer, sources=some)
    values, keys = ops.betweenness(ei, n, [0, n - 1, 0])
    assert set(sub) == {ids[i] for i in np.nonzero(keys)[0]}
    np.testing.assert_allclose([sub[i] if i in sub else 0.0 for i in ids], values, **TOL)


def test_rolling_time_window_item_and_aggregate():
    t = pp.TemporalGraph.from_edge_list(REFERENCE_EXAMPLE, device=DEV)
    items = list(pp.algorithms.RollingTimeWindow(t, 10, 10, return_window=True))
    g, window = items[2]
    assert window == (21, 31) and g.data.edge_index.size(1) == 6
    ids = [g.mapping.to_id(i) for i in range(g.n)]
    check_graph(g, g.data.edge_index.cpu().numpy(), g.n, ids=ids)
    static = t.to_static_graph()
    ids = [static.mapping.to_id(i) for i in range(static.n)]
    check_graph(static, static.data.edge_index.cpu().numpy(), static.n, ids=ids)
    assert set(pp.algorithms.betweenness_centrality(static)) <= set("abcdefghi")


def test_path_node_traversals_on_the_device():
    paths = pp.PathData(mapping=pp.IndexMap(["A", "B", "C", "D", "E", "F"]), device=DEV)
    paths.append_walk(("C", "B", "D", "F"), weight=1.0)
    paths.append_walk(("A", "B", "D"), weight=1.0)
    paths.append_walk(("D", "E"), weight=1.0)
    assert ct.path_node_traversals(paths) == {"A": 1, "B": 2, "C": 1, "D": 3, "E": 1, "F": 1}
    assert ct.path_visitation_probabilities(paths)["D"] == 3 / 9
