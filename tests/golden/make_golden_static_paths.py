#!/usr/bin/env python3
"""Generate tests/golden/static_paths_vectors.npz from the REFERENCE's own ``betweenness_centrality`` source, scipy and networkx.

Run where a checkout of the reference, scipy and networkx exist; no test needs any of them for the fixtures.  ``import pathpyG`` needs
torch_geometric, which this project does not depend on, so the one function is loaded from its source file by name with ``ast`` — the route make_golden.py
takes — and run on a duck-typed graph that offers what it reads: ``nodes`` and ``successors(v)`` (every stored edge of the row-sorted
edge list, parallel edges and self-loops included, as the reference's ``Graph.successors`` slices them out of its CSR).  The distances
come from ``scipy.sparse.csgraph.dijkstra(..., unweighted=True)`` and closeness from ``networkx.closeness_centrality`` on the DiGraph
of the edge list, the two calls the reference makes.  Nothing of the reference's text is written to the repository: only inputs and
the outputs its code produced for them.

    python tests/golden/make_golden_static_paths.py <path to the reference's src/pathpyG>

Per case ``<name>`` the file holds ``<name>/edge_index`` int64 [2, m] (row-sorted, stable), ``/n``, ``/undirected``, ``/dist`` int32 [n, n]
(-1 = inf), ``/bw`` float64 [n] and ``/bw_keys`` bool [n] (the keys of the returned dict), ``/closeness`` float64 [n], and for one
source list with a repeated entry ``/sources`` int64, ``/sub_bw``, ``/sub_bw_keys``; ``names`` lists the cases.
"""
from __future__ import annotations

import ast
import pathlib
import sys
from collections import defaultdict

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent


def load_reference_betweenness(ref: pathlib.Path):
    ns = {"defaultdict": defaultdict, "Graph": object}
    path = ref / "algorithms" / "centrality.py"
    for node in ast.parse(path.read_text()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "betweenness_centrality":
            exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), ns)  # noqa: S102 - the reference's own function
    return ns["betweenness_centrality"]


class DuckGraph:
    def __init__(self, edge_index: np.ndarray, n: int):
        order = np.argsort(edge_index[0], kind="stable")
        self.edge_index = edge_index[:, order]
        self.n = n
        self.nodes = list(range(n))
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(edge_index[0], minlength=n), out=ptr[1:])
        self._rows = [self.edge_index[1, ptr[v]:ptr[v + 1]].tolist() for v in range(n)]

    def successors(self, v):
        return self._rows[v]


def undirected(pairs) -> np.ndarray:
    """Both directions of every pair, parallel edges merged, (row, col)-sorted: what Graph.to_undirected() stores."""
    both = {(u, v) for u, v in pairs} | {(v, u) for u, v in pairs}
    return np.array(sorted(both), dtype=np.int64).T.reshape(2, -1)


def cases():
    a, b, c, d, e, f, g = range(7)
    toy = [(a, b), (b, c), (c, a), (d, e), (e, f), (f, g), (g, d), (d, f), (b, d)]
    yield "ref_triangle", undirected([(a, b), (b, c), (a, c)]), 3, True
    yield "ref_simple_graph_sp", undirected([(a, b), (b, c), (c, e), (b, d), (d, e)]), 5, True
    yield "ref_toy_undirected", undirected(toy), 7, True
    yield "ref_toy_directed", np.array(toy, dtype=np.int64).T, 7, False
    rng = np.random.default_rng(20240607)
    for i in range(48):                                             # multigraphs: parallel edges and self-loops on purpose
        n = int(rng.integers(2, 15))
        m = int(rng.integers(0, 3 * n + 1))
        ei = rng.integers(0, n, (2, m))
        if m >= 4:
            ei[:, 1] = ei[:, 0]                                     # a parallel edge
            ei[1, 2] = ei[0, 2]                                     # a self-loop
        yield f"random_{i:02d}", ei.astype(np.int64), n, False
    side = 12
    grid = [(r * side + q, r * side + q + 1) for r in range(side) for q in range(side - 1)]
    grid += [(r * side + q, (r + 1) * side + q) for r in range(side - 1) for q in range(side)]
    yield "grid_12x12", undirected(grid), side * side, True
    layers = 40                                                     # sigma doubles per layer after the first: 2^38 paths into the last one
    dag = [(2 * k + i, 2 * k + 2 + j) for k in range(layers - 1) for i in range(2) for j in range(2)]
    yield "dag_40x2", np.array(dag, dtype=np.int64).T, 2 * layers, False
    comp = [(0, 1), (1, 2), (2, 0), (2, 3), (5, 6), (6, 7), (7, 5), (6, 5)]           # two components; nodes 4, 8, 9 isolated
    yield "two_components_isolated", np.array(comp, dtype=np.int64).T, 10, False


def main() -> int:
    import networkx as nx
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra

    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    ref = pathlib.Path(sys.argv[1])
    reference_bw = load_reference_betweenness(ref)
    rng = np.random.default_rng(7)
    store, names = {}, []
    for name, ei, n, is_undirected in cases():
        graph = DuckGraph(ei, n)
        ei = graph.edge_index
        adj = coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
        dist = dijkstra(adj, directed=not is_undirected, return_predecessors=False, unweighted=True)
        nxg = nx.DiGraph()
        nxg.add_nodes_from(range(n))
        nxg.add_edges_from(ei.T.tolist())
        closeness = nx.closeness_centrality(nxg)
        bw = reference_bw(graph)
        sources = rng.integers(0, n, 3).tolist()
        sources.append(sources[0])                                  # a repeated source counts twice
        sub = reference_bw(graph, sources)
        store[f"{name}/edge_index"] = ei
        store[f"{name}/n"] = np.int64(n)
        store[f"{name}/undirected"] = np.bool_(is_undirected)
        store[f"{name}/dist"] = np.where(np.isfinite(dist), dist, -1).astype(np.int32)
        store[f"{name}/bw"] = np.array([float(bw[v]) if v in bw else 0.0 for v in range(n)])
        store[f"{name}/bw_keys"] = np.array([v in bw for v in range(n)])
        store[f"{name}/closeness"] = np.array([closeness[v] for v in range(n)])
        store[f"{name}/sources"] = np.array(sources, dtype=np.int64)
        store[f"{name}/sub_bw"] = np.array([float(sub[v]) if v in sub else 0.0 for v in range(n)])
        store[f"{name}/sub_bw_keys"] = np.array([v in sub for v in range(n)])
        names.append(name)
    store["names"] = np.array(names)
    np.savez_compressed(OUT / "static_paths_vectors.npz", **store)
    print(f"{len(names)} cases -> {OUT / 'static_paths_vectors.npz'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
