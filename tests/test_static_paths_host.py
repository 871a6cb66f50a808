"""Static shortest paths / centralities without a device: the plain restatement (tests/cpu_ops_static_paths.py) reproduces every fixture
made from the reference's own function, scipy and networkx (tests/golden/make_golden_static_paths.py), the reference's known answers hold,
and the host logic of the public functions — id handling, the single-node values, closeness from totals — needs no GPU.

Tolerance of the betweenness values: 1e-10 relative, 1e-10 absolute at zero.  All terms are non-negative, so another summation order
moves a sum by at most (number of additions) * 2^-53 relative, and no sum of these cases has more than 10^6 terms.
dist, closeness and the key sets are exact."""
import math
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_static_paths as ops
import pathpyg_amd as pp
from pathpyg_amd.algorithms import centrality, shortest_paths

GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "static_paths_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]
TOL = dict(rtol=1e-10, atol=1e-10)


def case(name):
    get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
    dist = get("dist").astype(np.float64)
    dist[dist < 0] = np.inf
    return dict(edge_index=get("edge_index"), n=int(get("n")), dist=dist, bw=get("bw"), bw_keys=get("bw_keys"), closeness=get("closeness"),
                sources=get("sources").tolist(), sub_bw=get("sub_bw"), sub_bw_keys=get("sub_bw_keys"))


def test_fixture_file_holds_the_cases_and_stays_small():
    assert {"ref_triangle", "ref_simple_graph_sp", "ref_toy_undirected", "ref_toy_directed", "grid_12x12", "dag_40x2",
            "two_components_isolated"} <= set(NAMES)
    assert sum(n.startswith("random_") for n in NAMES) >= 24
    assert (pathlib.Path(__file__).resolve().parent / "golden" / "static_paths_vectors.npz").stat().st_size < 400 * 1024
    dag = case("dag_40x2")
    assert dag["dist"][0, 78] == 39 and np.isinf(dag["dist"][78, 0])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_fixture(name):
    c = case(name)
    dist, pred = ops.shortest_paths(c["edge_index"], c["n"])
    assert np.array_equal(dist, c["dist"])
    assert np.array_equal(ops.closeness(dist), c["closeness"])
    values, keys = ops.betweenness(c["edge_index"], c["n"])
    assert np.array_equal(keys, c["bw_keys"])
    np.testing.assert_allclose(values, c["bw"], **TOL)
    values, keys = ops.betweenness(c["edge_index"], c["n"], c["sources"])
    assert np.array_equal(keys, c["sub_bw_keys"])
    np.testing.assert_allclose(values, c["sub_bw"], **TOL)
    # predecessors: valid, and the largest tight index
    edges = set(map(tuple, c["edge_index"].T.tolist()))
    for i in range(c["n"]):
        for j in range(c["n"]):
            p = int(pred[i, j])
            if i == j or np.isinf(dist[i, j]):
                assert p == ops.NO_PRED
            else:
                assert dist[i, p] + 1 == dist[i, j] and (p, j) in edges
                assert p == max(u for (u, v) in edges if v == j and dist[i, u] + 1 == dist[i, j])


@pytest.mark.parametrize("name", NAMES)
def test_all_sources_form_equals_the_per_source_loops(name):
    c = case(name)
    dist, pred = ops.shortest_paths(c["edge_index"], c["n"])
    values, keys = ops.betweenness(c["edge_index"], c["n"])
    got = ops.all_sources(c["edge_index"], c["n"])
    assert np.array_equal(got["dist"], dist) and np.array_equal(got["pred"], pred) and np.array_equal(got["keys"], keys)
    np.testing.assert_allclose(got["bw"], values, **TOL)
    sub = ops.all_sources(c["edge_index"], c["n"], c["sources"])
    assert np.array_equal(sub["keys"], c["sub_bw_keys"])
    np.testing.assert_allclose(sub["bw"], c["sub_bw"], **TOL)


def test_dag_path_counts_are_large_and_exact_in_float64():
    c = case("dag_40x2")
    row_ptr, col = ops.csr(c["edge_index"], c["n"])
    sigma = [0] * c["n"]
    sigma[0] = 1
    for v in range(c["n"]):
        for w in col[row_ptr[v]:row_ptr[v + 1]].tolist():
            sigma[w] += sigma[v]
    assert sigma[-1] == 2 ** 38 and 2 * sigma[-1] < 2 ** 53          # 39 layers below node 0's: each doubles the count but the first
    assert float(sigma[-1]) == sigma[-1]


def test_reference_known_answers():
    tri = case("ref_triangle")
    values, keys = ops.betweenness(tri["edge_index"], 3)
    assert keys.all() and values.tolist() == [0.0, 0.0, 0.0] and tri["bw"].tolist() == [0.0, 0.0, 0.0] and tri["bw_keys"].all()
    assert ops.closeness(tri["dist"]).tolist() == [1.0, 1.0, 1.0] and tri["closeness"].tolist() == [1.0, 1.0, 1.0]
    sp = case("ref_simple_graph_sp")
    want = np.array([[0, 1, 2, 2, 3], [1, 0, 1, 1, 2], [2, 1, 0, 2, 1], [2, 1, 2, 0, 1], [3, 2, 1, 1, 0]], dtype=np.float64)
    dist, _ = ops.shortest_paths(sp["edge_index"], 5)
    assert np.array_equal(dist, want) and np.array_equal(sp["dist"], want)
    assert ops.diameter(dist) == 3 and ops.avg_path_length(dist) == 1.6


def random_multigraph(rng, n_max=40):
    n = int(rng.integers(1, n_max))
    m = int(rng.integers(0, 4 * n))
    return rng.integers(0, n, (2, m)).astype(np.int64), n


def test_restatement_against_scipy_on_fresh_graphs():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(11)
    for _ in range(40):
        ei, n = random_multigraph(rng)
        adj = sparse.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
        want, want_pred = csgraph.dijkstra(adj, directed=True, return_predecessors=True, unweighted=True)
        dist, pred = ops.shortest_paths(ei, n)
        assert np.array_equal(dist, want)
        assert np.array_equal(pred == ops.NO_PRED, want_pred == ops.NO_PRED)
        assert ops.diameter(dist) == (float(np.max(want)) if n > 1 else 0.0)
        if n > 1:
            assert ops.avg_path_length(dist) == np.sum(want) / (n * (n - 1))


def test_restatement_against_networkx_closeness_on_fresh_graphs():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(12)
    for _ in range(40):
        ei, n = random_multigraph(rng)
        g = nx.DiGraph()
        g.add_nodes_from(range(n))
        g.add_edges_from(ei.T.tolist())
        want = nx.closeness_centrality(g)
        dist, _ = ops.shortest_paths(ei, n)
        assert ops.closeness(dist).tolist() == [want[v] for v in range(n)]
        reach_in, dist_in, _, _, _ = ops.totals(dist)
        assert centrality.closeness_from_totals(reach_in.tolist(), dist_in.tolist(), n) == [want[v] for v in range(n)]


# ------------------------------------------------------------------ host logic of the public functions
def host_graph(ids, edges=((), ())):
    """A Graph that needs no device to build: row-sorted edges and a known node count."""
    ei = torch.tensor([list(edges[0]), list(edges[1])], dtype=torch.int64).reshape(2, -1)
    return pp.Graph(pp.Data(edge_index=ei, num_nodes=len(ids)), mapping=pp.IndexMap(list(ids)), _row_sorted=True)


def test_modules_are_exposed_like_the_reference():
    assert pp.algorithms.shortest_paths is shortest_paths and pp.algorithms.centrality is centrality
    for name in ("shortest_paths_dijkstra", "diameter", "avg_path_length"):
        assert callable(getattr(shortest_paths, name))
    for name in ("betweenness_centrality", "closeness_centrality", "map_to_nodes", "path_node_traversals", "path_visitation_probabilities",
                 "temporal_betweenness_centrality", "temporal_closeness_centrality"):
        assert callable(getattr(centrality, name))
    assert centrality.temporal_betweenness_centrality is pp.algorithms.temporal_betweenness_centrality
    with pytest.raises(AttributeError):          # the reference forwards unknown names to networkx; this package does not
        centrality.degree_centrality


def test_map_to_nodes():
    g = host_graph(["a", "b", "c"], ((1, 1, 2), (0, 2, 1)))
    assert centrality.map_to_nodes(g, {0: 0.5, 1: 2.7, 2: 0.3}) == {"a": 0.5, "b": 2.7, "c": 0.3}
    assert centrality.map_to_nodes(g, {2: 1.0}) == {"c": 1.0}


def test_source_ids_keep_order_and_repeats_and_unknown_ids_raise():
    g = host_graph(["a", "b", "c"], ((1, 1, 2), (0, 2, 1)))
    assert centrality.source_indices(g, None) is None
    assert centrality.source_indices(g, ["c", "a", "c"]) == [2, 0, 2]
    with pytest.raises(KeyError):
        g.mapping.to_idx("z")
    with pytest.raises(KeyError):
        centrality.betweenness_centrality(g, sources=["a", "z"])
    assert dict(centrality.betweenness_centrality(g, sources=[])) == {}


def test_single_node_values_need_no_device():
    g = host_graph(["a"])
    assert shortest_paths.diameter(g) == 0.0
    assert math.isnan(shortest_paths.avg_path_length(g))
    assert centrality.closeness_centrality(g) == {"a": 0.0}


def test_without_a_device_every_search_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g = host_graph(["a", "b", "c"], ((1, 1, 2), (0, 2, 1)))
    for call in (shortest_paths.shortest_paths_dijkstra, shortest_paths.diameter, shortest_paths.avg_path_length,
                 centrality.closeness_centrality, centrality.betweenness_centrality):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(g)


def test_sizes_of_2_to_the_31_or_more_are_refused_before_any_launch():
    from pathpyg_amd import _lib
    L = _lib.lib()
    ok, too_large, workspace = 0, -4, -3                     # enum pp_status
    for n, m in ((2 ** 31, 10), (10, 2 ** 31)):
        assert L.pp_graph_bfs(None, None, n, m, None, 1, None, None, None, None, None, None, 0, None) == too_large
        assert L.pp_graph_betweenness(None, None, n, m, None, 1, None, None, None, 0, None) == too_large
    # 2^31 - 1 passes the size check: the next one (an empty workspace) answers
    assert L.pp_graph_bfs(None, None, 2 ** 31 - 1, 2 ** 31 - 1, None, 1, None, None, None, None, None, None, 0, None) == workspace
    assert L.pp_graph_betweenness(None, None, 2 ** 31 - 1, 2 ** 31 - 1, None, 1, None, None, None, 0, None) == workspace
    assert L.pp_graph_bfs(None, None, 0, 0, None, 0, None, None, None, None, None, None, 1 << 20, None) == ok
    assert L.pp_graph_bfs_parts(10, 5) == 5 and L.pp_graph_bfs_parts(5000, 5000) == 2048 and L.pp_graph_betweenness_parts(5000, 5000) == 1024


def test_closeness_from_totals_order_of_operations():
    # (r / tot) * (r / (n - 1)), not r * r / (tot * (n - 1)): the two differ in the last bit for these totals
    r, tot, n = 7, 11, 10
    assert centrality.closeness_from_totals([r, 0], [tot, 0], n) == [(r / tot) * (r / (n - 1)), 0.0]
    assert centrality.closeness_from_totals([0], [0], 1) == [0.0]


def test_path_helpers_on_host_path_data():
    paths = pp.PathData(mapping=pp.IndexMap(["A", "B", "C", "D", "E", "F"]))
    paths.append_walk(("C", "B", "D", "F"), weight=1.0)
    paths.append_walk(("A", "B", "D"), weight=1.0)
    paths.append_walk(("D", "E"), weight=1.0)
    assert centrality.path_node_traversals(paths) == {"A": 1, "B": 2, "C": 1, "D": 3, "E": 1, "F": 1}
    prob = centrality.path_visitation_probabilities(paths)
    assert prob == {"A": 1 / 9, "B": 2 / 9, "C": 1 / 9, "D": 3 / 9, "E": 1 / 9, "F": 1 / 9}
