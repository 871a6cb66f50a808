#!/usr/bin/env python3
"""Generate tests/golden/components_vectors.npz from scipy and the REFERENCE's own ``largest_connected_component`` source.

Run where a checkout of the reference and scipy exist; no test needs either for the fixtures.  ``import pathpyG`` needs torch_geometric,
which this project does not depend on, so the one function is loaded from its source file by name with ``ast`` — the route
make_golden_static_paths.py takes — and run on a duck-typed graph that offers what it reads: ``sparse_adj_matrix()`` (the coo matrix of
ones the reference's Graph builds), ``is_directed()`` / ``is_undirected()``, ``edges`` (ID pairs in stored order), ``mapping.to_idx`` and,
under the name ``Graph``, a ``from_edge_list`` that records its arguments.  The labels come from
``scipy.sparse.csgraph.connected_components`` on that matrix, the call the reference makes.  Nothing of the reference's text is written
to the repository: only inputs and the outputs its code produced for them.

    python tests/golden/make_golden_components.py <path to the reference's src/pathpyG>

Per case ``<name>`` the file holds ``<name>/edge_index`` int64 [2, m] (row-sorted, stable), ``/n``, ``/weak`` and ``/strong`` int32 [n]
(scipy's labels of the directed graph), ``/undirected`` int32 [n] (``directed=False``: what a graph flagged undirected gets for either
``connection``), and for ``<kind>`` in weak, strong, undirected ``/lcc_<kind>`` int64 [2, k]: the edge list the reference handed to
``from_edge_list``, as node indices, with ``/lcc_<kind>_label`` the label it chose.  Node IDs are ``v000, v001, ...`` (``"v%03d" % index``:
above 999 their sorted order is not the index order).  ``names`` lists the cases.
"""
from __future__ import annotations

import ast
import pathlib
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from make_golden_static_paths import cases as static_path_cases  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent


class Recorder:
    calls: list = []

    @staticmethod
    def from_edge_list(edge_list, is_undirected=False, **kw):
        Recorder.calls.append((list(edge_list), bool(is_undirected)))
        return Recorder.calls[-1]


def load_reference_lcc(ref: pathlib.Path):
    from scipy.sparse.csgraph import connected_components

    ns = {"Counter": Counter, "_cc": connected_components, "_np": np, "Graph": Recorder, "Tuple": tuple}
    path = ref / "algorithms" / "components.py"
    for node in ast.parse(path.read_text()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "largest_connected_component":
            exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), ns)  # noqa: S102 - the reference's own function
    return ns["largest_connected_component"]


class DuckMapping:
    def __init__(self, ids):
        self._idx = {x: i for i, x in enumerate(ids)}

    def to_idx(self, node):
        return self._idx[node]


class DuckGraph:
    def __init__(self, edge_index: np.ndarray, n: int, undirected: bool):
        order = np.argsort(edge_index[0], kind="stable")
        self.edge_index = edge_index[:, order]
        self.n = n
        self._undirected = undirected
        self.ids = [f"v{i:03d}" for i in range(n)]
        self.mapping = DuckMapping(self.ids)
        self.edges = [(self.ids[u], self.ids[w]) for u, w in self.edge_index.T.tolist()]

    def is_directed(self):
        return not self._undirected

    def is_undirected(self):
        return self._undirected

    def sparse_adj_matrix(self):
        from scipy.sparse import coo_matrix
        ei = self.edge_index
        return coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(self.n, self.n))


def cases():
    for name, ei, n, _ in static_path_cases():
        if name.startswith(("ref_", "random_")) or name == "two_components_isolated":
            yield name, ei, n
    rng = np.random.default_rng(20241020)
    for m in (1100, 3000, 8000):                                    # many small components / a strong giant among singletons / one giant
        yield f"big_2000_{m}", rng.integers(0, 2000, (2, m)).astype(np.int64), 2000


def main() -> int:
    from scipy.sparse.csgraph import connected_components

    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    reference_lcc = load_reference_lcc(pathlib.Path(sys.argv[1]))
    store, names = {}, []
    for name, ei, n in cases():
        directed, flagged = DuckGraph(ei, n, False), DuckGraph(ei, n, True)
        store[f"{name}/edge_index"] = directed.edge_index
        store[f"{name}/n"] = np.int64(n)
        adj = directed.sparse_adj_matrix()
        labels = {"weak": connected_components(adj, directed=True, connection="weak")[1],
                  "strong": connected_components(adj, directed=True, connection="strong")[1],
                  "undirected": connected_components(adj, directed=False, connection="strong")[1]}
        for kind, lab in labels.items():
            store[f"{name}/{kind}"] = lab.astype(np.int32)
            graph = flagged if kind == "undirected" else directed
            Recorder.calls.clear()
            reference_lcc(graph, connection="weak" if kind == "weak" else "strong")
            (edges, is_undirected), = Recorder.calls
            assert is_undirected == (kind == "undirected")
            kept = np.array([[graph.mapping.to_idx(v), graph.mapping.to_idx(w)] for v, w in edges], dtype=np.int64).reshape(-1, 2).T
            chosen = Counter(lab.tolist()).most_common(1)[0][0]
            assert (lab[kept] == chosen).all()
            store[f"{name}/lcc_{kind}"] = kept
            store[f"{name}/lcc_{kind}_label"] = np.int64(chosen)
        names.append(name)
        if name.startswith("big_"):
            for kind, lab in labels.items():
                print(f"{name} {kind}: {lab.max() + 1} components, largest {np.bincount(lab).max()}")
    store["names"] = np.array(names)
    np.savez_compressed(OUT / "components_vectors.npz", **store)
    print(f"{len(names)} cases -> {OUT / 'components_vectors.npz'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
