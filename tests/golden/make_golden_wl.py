#!/usr/bin/env python3
"""Generate tests/golden/wl_vectors.npz from the REFERENCE's own ``WeisfeilerLeman_test`` source.

Run where a checkout of the reference exists; no test needs it for the fixtures.  ``import pathpyG`` needs torch_geometric, which this
project does not depend on, so the one function is loaded from its source file by name with ``ast`` — the route
make_golden_components.py takes — and run on duck-typed graphs that offer what it reads: ``mapping.node_ids``, ``nodes``,
``successors(node)`` and ``__add__`` (the union with the ``np.unique(..., axis=0)`` node order of the reference's ``Graph.__add__``, the
edges of the first graph before those of the second).  Nothing of the reference's text is written to the repository: only inputs and the
outputs its code produced for them.

    python tests/golden/make_golden_wl.py <path to the reference's src/pathpyG>

Per case ``<name>`` and graph ``<g>`` in 1, 2 the file holds ``<name>/ids<g>`` (the node IDs in index order: strings, or a 2-D array of
strings for tuple IDs), ``<name>/edge_index<g>`` int64 [2, m] (node indices, row-sorted, stable) and, if the case has features,
``<name>/feat<g>`` int64 [n]: codes into ``<name>/feat_values`` (strings), with ``<name>/feat_int`` = 1 when the values are the decimal
forms of integer features.  Outputs: ``<name>/result`` (bool), ``<name>/fp<g>`` int64 [n] and ``<name>/fp_initial``: 0 when the
fingerprints are the integer labels themselves, 1 when the function returned the INITIAL fingerprint — ``fp<g>`` then holds codes into
``feat_values``, or zeros for the string ``'0'`` of a run without features.  ``names`` lists the cases.
"""
from __future__ import annotations

import ast
import pathlib
import sys

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent


def load_reference_test(ref: pathlib.Path):
    ns = {"Dict": dict, "List": list, "Tuple": tuple, "Graph": object}
    path = ref / "algorithms" / "weisfeiler_leman.py"
    for node in ast.parse(path.read_text()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "WeisfeilerLeman_test":
            node.returns = None
            for arg in node.args.args:
                arg.annotation = None
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), str(path), "exec"), ns)  # noqa: S102 - the reference's own function
    return ns["WeisfeilerLeman_test"]


class DuckMapping:
    def __init__(self, ids):
        self.node_ids = list(ids)


class DuckGraph:
    """``ids``: the node IDs in index order (strings or tuples of strings); ``pairs``: stored edges as index pairs."""

    def __init__(self, ids, pairs):
        self.nodes = list(ids)
        self.mapping = DuckMapping(self.nodes)
        ei = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T
        self.edge_index = ei[:, np.argsort(ei[0], kind="stable")]
        self._succ = {v: [] for v in self.nodes}
        for u, w in self.edge_index.T.tolist():
            self._succ[self.nodes[u]].append(self.nodes[w])

    def successors(self, node):
        return list(self._succ[node])

    def __add__(self, other):
        merged = np.unique(np.concatenate([np.asarray(self.nodes), np.asarray(other.nodes)]), axis=0).tolist()
        union = object.__new__(DuckGraph)
        union.nodes = [tuple(x) for x in merged] if merged and isinstance(merged[0], list) else merged
        union.mapping = DuckMapping(union.nodes)
        union._succ = {**self._succ, **other._succ}
        return union


def from_edge_list(edges, undirected=False):
    """IDs in sorted order, as Graph.from_edge_list indexes them; ``undirected``: both directions of every edge, (row, col)-sorted."""
    ids = sorted({v for e in edges for v in e})
    idx = {v: i for i, v in enumerate(ids)}
    pairs = [(idx[u], idx[w]) for u, w in edges]
    if undirected:
        pairs = sorted(set(pairs) | {(w, u) for u, w in pairs})
    return DuckGraph(ids, pairs)


def ring(ids):
    k = len(ids)
    return [(ids[i], ids[(i + 1) % k]) for i in range(k)]


def cases():
    """``(name, g1, g2, features_g1, features_g2)``"""
    yield "ref_1", from_edge_list([("a", "b"), ("b", "c")]), from_edge_list([("y", "z"), ("x", "y")]), None, None
    yield "ref_2", from_edge_list([("a", "b"), ("b", "c")]), from_edge_list([("y", "z"), ("x", "z")]), None, None
    cube_a = [("a", "g"), ("a", "h"), ("a", "i"), ("b", "g"), ("b", "h"), ("b", "j"), ("c", "g"), ("c", "i"), ("c", "j"), ("d", "h"), ("d", "i"),
              ("d", "j")]
    cube_b = [("1", "2"), ("1", "5"), ("1", "4"), ("2", "6"), ("2", "3"), ("3", "7"), ("3", "4"), ("4", "8"), ("5", "6"), ("6", "7"), ("7", "8"),
              ("8", "5")]
    yield "ref_3", from_edge_list(cube_a, True), from_edge_list(cube_b, True), None, None
    yield ("triangles_hexagon", from_edge_list(ring(["a", "b", "c"]) + ring(["d", "e", "f"]), True),
           from_edge_list(ring(["u", "v", "w", "x", "y", "z"]), True), None, None)
    yield ("directed_sinks_sources", from_edge_list([("a", "b"), ("a", "c"), ("b", "d"), ("c", "d"), ("e", "a")]),
           from_edge_list([("p", "q"), ("p", "r"), ("q", "s"), ("r", "s"), ("s", "t")]), None, None)
    yield ("parallel_edges", DuckGraph(["h", "a", "b"], [(0, 1), (0, 1), (0, 2), (1, 2)]),
           DuckGraph(["k", "x", "y"], [(0, 1), (0, 2), (0, 2), (1, 2)]), None, None)
    yield ("self_loops", DuckGraph(["a", "b", "c"], [(0, 0), (0, 1), (1, 2), (2, 2)]),
           DuckGraph(["x", "y", "z"], [(0, 1), (1, 1), (1, 2), (2, 2)]), None, None)
    yield ("isolated_nodes", DuckGraph(["a", "b", "c", "d", "e"], [(0, 1), (1, 0)]),
           DuckGraph(["v", "w", "x", "y", "z"], [(4, 2), (2, 4)]), None, None)
    yield "unequal_sizes", from_edge_list(ring(["a", "b", "c", "d"]), True), from_edge_list(ring(["v", "w", "x", "y", "z"]), True), None, None
    # sorted union: a1 b1 a2 b2 ... — the first occurrences of the classes alternate between the graphs
    yield ("interleaved_ids", DuckGraph(["n1", "n3", "n5", "n7"], [(0, 1), (1, 2), (2, 3), (0, 2)]),
           DuckGraph(["n6", "n4", "n2", "n0"], [(0, 1), (1, 2), (2, 3), (0, 2)]), None, None)
    yield ("interleaved_ids_false", DuckGraph(["n1", "n3", "n5", "n7"], [(0, 1), (1, 2), (2, 3), (0, 2)]),
           DuckGraph(["n6", "n4", "n2", "n0"], [(0, 1), (1, 2), (2, 3), (1, 3)]), None, None)
    yield ("tuple_ids", DuckGraph([("a", "b"), ("b", "c"), ("c", "a"), ("b", "a")], [(0, 1), (1, 2), (2, 0), (3, 0), (0, 3)]),
           DuckGraph([("x", "z"), ("a", "a"), ("y", "x"), ("c", "b")], [(0, 2), (2, 1), (1, 0), (3, 0), (0, 3)]), None, None)
    path_a, path_b = from_edge_list([("a", "b"), ("b", "c"), ("c", "d")]), from_edge_list([("w", "x"), ("x", "y"), ("y", "z")])
    yield ("string_features", path_a, path_b, {"a": "red", "b": "blue", "c": "red", "d": "blue"},
           {"w": "red", "x": "blue", "y": "red", "z": "blue"})
    yield ("string_features_false", path_a, path_b, {"a": "red", "b": "blue", "c": "red", "d": "blue"},
           {"w": "blue", "x": "red", "y": "red", "z": "blue"})
    yield ("string_features_stable", from_edge_list(ring(["a", "b"])), from_edge_list(ring(["y", "z"])), {"a": "p", "b": "q"}, {"y": "q", "z": "p"})
    # '1' on the sink that comes first in sorted order: round 1 numbers its label "1[]" 1, so every later round builds "1[]" for it again
    # and the dict hands the 1 out again instead of a new number
    chain_a, chain_b = from_edge_list([("e", "d"), ("d", "c"), ("c", "b"), ("b", "a")]), \
        from_edge_list([("z", "y"), ("y", "x"), ("x", "w"), ("w", "v")])
    yield ("feature_one_on_sink", chain_a, chain_b, {"a": "1", "b": "7", "c": "7", "d": "7", "e": "7"}, {"v": "1", "w": "7", "x": "7", "y": "7", "z": "7"})
    yield ("feature_one_everywhere", path_a, path_b, {v: "1" for v in "abcd"}, {v: "1" for v in "wxyz"})
    yield ("integer_features", path_a, path_b, {"a": 1, "b": 2, "c": 1, "d": 2}, {"w": 1, "x": 2, "y": 1, "z": 2})
    yield ("integer_features_reuse", chain_a, chain_b, {"a": 1, "b": 3, "c": 3, "d": 3, "e": 3}, {"v": 1, "w": 3, "x": 3, "y": 3, "z": 3})
    rng = np.random.default_rng(20241021)
    for i in range(6):                                                  # random multigraphs; the second one a relabelled copy on even i
        n = int(rng.integers(5, 13))
        m = int(rng.integers(n, 3 * n))
        pairs = rng.integers(0, n, (m, 2)).tolist()
        perm = rng.permutation(n)
        other = [(int(perm[u]), int(perm[w])) for u, w in pairs] if i % 2 == 0 else rng.integers(0, n, (m, 2)).tolist()
        yield (f"random_{i}", DuckGraph([f"a{j:02d}" for j in range(n)], pairs), DuckGraph([f"a{j:02d}x" for j in range(n)], other), None, None)


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    reference_test = load_reference_test(pathlib.Path(sys.argv[1]))
    store, names = {}, []
    for name, g1, g2, f1, f2 in cases():
        result, fp1, fp2 = reference_test(g1, g2, f1, f2)
        values = []
        if f1 is not None:
            merged = {**f1, **f2}
            values = sorted({str(x) for x in merged.values()})
            store[f"{name}/feat_values"] = np.array(values)
            store[f"{name}/feat_int"] = np.int64(all(isinstance(x, int) for x in merged.values()))
            for g, graph in (("1", g1), ("2", g2)):
                store[f"{name}/feat{g}"] = np.array([values.index(str(merged[v])) for v in graph.nodes], dtype=np.int64)
        every = fp1 + fp2
        merged_values = list({**f1, **f2}.values()) if f1 is not None else []
        initial = all(x == "0" for x in every) if f1 is None else all(type(x) is type(merged_values[0]) and x in merged_values for x in every) \
            and [*fp1, *fp2] == [{**f1, **f2}[v] for v in g1.nodes + g2.nodes]
        if not initial:
            assert all(type(x) is int for x in every), (name, every)
        for g, graph, fp in (("1", g1, fp1), ("2", g2, fp2)):
            store[f"{name}/ids{g}"] = np.array(graph.nodes)
            store[f"{name}/edge_index{g}"] = graph.edge_index
            if initial:
                fp = [values.index(str(x)) for x in fp] if f1 is not None else [0] * len(fp)
            store[f"{name}/fp{g}"] = np.array(fp, dtype=np.int64)
        store[f"{name}/result"] = np.bool_(result)
        store[f"{name}/fp_initial"] = np.int64(initial)
        names.append(name)
        print(f"{name}: {result} initial={int(initial)} largest={max([x for x in every if type(x) is int], default='-')}")
    store["names"] = np.array(names)
    np.savez_compressed(OUT / "wl_vectors.npz", **store)
    print(f"{len(names)} cases -> {OUT / 'wl_vectors.npz'}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
