#!/usr/bin/env python3
"""Generate tests/golden/statistics_vectors.npz from the REFERENCE's own ``pathpyG.statistics`` sources.

Run where a checkout of the reference, torch and scipy exist; no test needs the reference for the fixtures.  ``import pathpyG`` needs
torch_geometric, which this project does not depend on, so every function of ``statistics/{clustering,degrees,node_similarities}.py`` is
loaded from its source file by name with ``ast`` — the route make_golden_components.py takes — and run on a duck-typed graph that offers
what they read: ``successors``, ``nodes``, ``n``, ``m``, ``is_directed`` / ``is_undirected``, ``degrees(mode, return_tensor)``,
``out_degrees``, ``data.edge_index``, ``mapping.to_idx`` and ``sparse_adj_matrix``, each restating what the reference's Graph does on a
row-sorted stored edge list (parallel edges and self-loops kept).  ``shortest_paths_dijkstra`` is the scipy call the reference makes.
Nothing of the reference's text is written to the repository: only inputs and the outputs its code produced for them.

    python tests/golden/make_golden_statistics.py <path to the reference's src/pathpyG>

Per case ``<name>`` the file holds ``/edge_index`` int64 [2, m] (row-sorted, stable), ``/n``, ``/undirected``; ``/triads`` int64 [n] (the sizes
of ``closed_triads``), ``/coeff`` float64 [n], ``/avg``; per ``<mode>`` in in, out, total: ``/<mode>/sequence`` int32 [n], ``/distribution``
float32, ``/genfun`` float32 [3] at x = [0, 0.3, 1], and ``/scalars`` float64 in the order of ``SCALARS`` below (raw and central moments
for k = 1, 2, 3, the mean degree, the mean neighbour degree without and with exclude_backlink, the assortativity, the generating function at
the float 0.3); and for all ordered pairs of the first ``k = min(n, 6)`` nodes ``/pair/values`` float64 [6, k, k] in the order of
``MEASURES`` below.  Where the reference raises ``ZeroDivisionError`` the value is ``nan`` and the int8 array ``/raised`` of the same shape
holds 1.
``ref_toy_undirected`` also holds ``/katz`` and ``/lhn`` float64 [2] for ("e", "g") at 0.02 and 0.2, the reference test's parameters.
Node IDs are ``v000, v001, ...``.  ``names`` lists the cases.
"""
from __future__ import annotations

import ast
import pathlib
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
from make_golden_static_paths import cases as static_path_cases, undirected  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent
MODES = ("in", "out", "total")
X = [0, 0.3, 1]
SCALARS = ("raw_1", "raw_2", "raw_3", "central_1", "central_2", "central_3", "mean", "neighbor", "neighbor_no_backlink", "assortativity",
           "genfun_0.3")
MEASURES = ("common_neighbors", "overlap_coefficient", "jaccard_similarity", "adamic_adar_index", "cosine_similarity", "inverse_path_length")


def load_reference(ref: pathlib.Path) -> dict:
    import scipy
    import scipy.sparse.linalg  # noqa: F401 - the reference reaches it as _sp.sparse.linalg
    from scipy.sparse.csgraph import dijkstra

    def shortest_paths_dijkstra(graph):
        return dijkstra(graph.sparse_adj_matrix(), directed=graph.is_directed(), return_predecessors=True, unweighted=True)

    ns = {"torch": torch, "_np": np, "_sp": scipy, "Graph": object, "Set": set, "shortest_paths_dijkstra": shortest_paths_dijkstra}
    for module in ("clustering", "degrees", "node_similarities"):
        path = ref / "statistics" / f"{module}.py"
        for node in ast.parse(path.read_text()).body:
            if isinstance(node, ast.FunctionDef):
                exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), ns)  # noqa: S102 - the reference's own function
    return ns


class DuckMapping:
    def __init__(self, ids):
        self._idx = {x: i for i, x in enumerate(ids)}

    def to_idx(self, node):
        return self._idx[node]


class DuckData:
    def __init__(self, edge_index):
        self.edge_index = torch.from_numpy(edge_index)


class DuckGraph:
    def __init__(self, edge_index: np.ndarray, n: int, is_undirected: bool):
        order = np.argsort(edge_index[0], kind="stable")
        self.edge_index = np.ascontiguousarray(edge_index[:, order])
        self.data = DuckData(self.edge_index)
        self.n = n
        self._undirected = is_undirected
        self.nodes = [f"v{i:03d}" for i in range(n)]
        self.mapping = DuckMapping(self.nodes)
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.edge_index[0], minlength=n), out=ptr[1:])
        self._rows = {self.nodes[v]: [self.nodes[w] for w in self.edge_index[1, ptr[v]:ptr[v + 1]]] for v in range(n)}

    def is_directed(self):
        return not self._undirected

    def is_undirected(self):
        return self._undirected

    def successors(self, v):
        return self._rows[v]

    @property
    def m(self):
        stored = self.edge_index.shape[1]
        if not self._undirected:
            return stored
        loops = int((self.edge_index[0] == self.edge_index[1]).sum())
        return int((stored - loops) / 2 + loops)

    def degrees(self, mode="in", edge_attr=None, return_tensor=False):
        d = torch.from_numpy(np.bincount(self.edge_index[1 if mode == "in" else 0], minlength=self.n).astype(np.int32))
        return d if return_tensor else {node: deg.item() for node, deg in zip(self.nodes, d)}

    @property
    def out_degrees(self):
        return self.degrees(mode="out")

    def sparse_adj_matrix(self):
        from scipy.sparse import coo_matrix
        ei = self.edge_index
        return coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(self.n, self.n))


def cases():
    yield from static_path_cases()
    yield "star_9", undirected([(0, leaf) for leaf in range(1, 10)]), 10, True
    yield "k8", undirected([(u, w) for u in range(8) for w in range(u + 1, 8)]), 8, True
    yield "cycle3_loop", np.array([(0, 1), (1, 2), (2, 0), (1, 1)], dtype=np.int64).T, 3, False
    yield "two_hubs", np.array([(hub, leaf) for hub in (0, 1) for leaf in range(2, 12)] + [(2, 0), (3, 1), (4, 5)], dtype=np.int64).T, 12, False


def guarded(fn, *args, **kw):
    """``(value, raised)``: nan and 1 where the reference raises ZeroDivisionError."""
    try:
        return float(fn(*args, **kw)), 0
    except ZeroDivisionError:
        return float("nan"), 1


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    ref = load_reference(pathlib.Path(sys.argv[1]))
    warnings.simplefilter("ignore", RuntimeWarning)                 # log(0), 1 / log(1), 0 / 0: the values are what is recorded
    store, names = {}, []
    for name, ei, n, is_undirected in cases():
        g = DuckGraph(ei, n, is_undirected)
        store[f"{name}/edge_index"] = g.edge_index
        store[f"{name}/n"] = np.int64(n)
        store[f"{name}/undirected"] = np.bool_(is_undirected)
        store[f"{name}/triads"] = np.array([len(ref["closed_triads"](g, v)) for v in g.nodes], dtype=np.int64)
        store[f"{name}/coeff"] = np.array([ref["local_clustering_coefficient"](g, v) for v in g.nodes], dtype=np.float64)
        store[f"{name}/avg"] = np.float64(ref["avg_clustering_coefficient"](g))
        for mode in MODES:
            key = f"{name}/{mode}"
            seq = ref["degree_sequence"](g, mode=mode)
            sums = [float(seq.double().pow(p).sum()) for p in (1, 2, 3)]
            sums.append(float((seq.double()[g.data.edge_index[0]] * seq.double()[g.data.edge_index[1]]).sum()))
            assert max(sums) < 2 ** 24, (name, mode, sums)          # every float32 sum of degree_assortativity is exact
            store[f"{key}/sequence"] = seq.numpy().astype(np.int32)
            store[f"{key}/distribution"] = ref["degree_distribution"](g, mode=mode).numpy()
            store[f"{key}/genfun"] = ref["degree_generating_function"](g, X, mode=mode).numpy()
            scalars = [(ref["degree_raw_moment"](g, k=k, mode=mode), 0) for k in (1, 2, 3)]
            scalars += [(ref["degree_central_moment"](g, k=k, mode=mode), 0) for k in (1, 2, 3)]
            scalars.append((ref["mean_degree"](g, mode=mode), 0))
            scalars += [guarded(ref["mean_neighbor_degree"], g, mode=mode, exclude_backlink=flag) for flag in (False, True)]
            scalars.append(guarded(ref["degree_assortativity"], g, mode=mode))
            scalars.append((ref["degree_generating_function"](g, 0.3, mode=mode), 0))
            assert len(scalars) == len(SCALARS)
            store[f"{key}/scalars"] = np.array([v for v, _ in scalars], dtype=np.float64)
            store[f"{key}/raised"] = np.array([r for _, r in scalars], dtype=np.int8)
        k = min(n, 6)
        values, raised = np.zeros((len(MEASURES), k, k)), np.zeros((len(MEASURES), k, k), dtype=np.int8)
        for i, fn in enumerate(MEASURES):
            for a in range(k):
                for b in range(k):
                    values[i, a, b], raised[i, a, b] = guarded(ref[fn], g, g.nodes[a], g.nodes[b])
        store[f"{name}/pair/values"] = values
        store[f"{name}/pair/raised"] = raised
        if name == "ref_toy_undirected":
            e, gg = g.nodes[4], g.nodes[6]
            store[f"{name}/katz"] = np.array([ref["katz_index"](g, e, gg, beta=b) for b in (0.02, 0.2)], dtype=np.float64)
            store[f"{name}/lhn"] = np.array([np.real(ref["LeichtHolmeNewman_index"](g, e, gg, alpha=a)) for a in (0.02, 0.2)], dtype=np.float64)
        names.append(name)
    store["names"] = np.array(names)
    np.savez_compressed(OUT / "statistics_vectors.npz", **store)
    print(f"{len(names)} cases -> {OUT / 'statistics_vectors.npz'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
