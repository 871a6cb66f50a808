"""Centralities of static and temporal graphs, HIP-backed (reference ``pathpyG.algorithms.centrality``).

```py
import pathpyg_amd as pp

g = pp.TemporalGraph.from_edge_list([('b', 'c', 2), ('a', 'b', 1), ('c', 'd', 3), ('d', 'a', 4), ('b', 'd', 2), ('d', 'a', 6), ('a', 'b', 7)])
bw_t = pp.algorithms.centrality.temporal_betweenness_centrality(g, delta=1)
cl_t = pp.algorithms.centrality.temporal_closeness_centrality(g, delta=1)

static_graph = g.to_static_graph()
bw_s = pp.algorithms.centrality.betweenness_centrality(static_graph)
cl_s = pp.algorithms.centrality.closeness_centrality(static_graph)
```

The static functions run breadth-first searches on the graph's CSR on the GPU (``pp_graph_bfs`` / ``pp_graph_betweenness``,
csrc/pp_graph_paths.hip); the temporal ones live in :mod:`pathpyg_amd.algorithms.temporal` and are re-exported here.  They take any
:class:`~pathpyg_amd.core.graph.Graph` on any device; edge weights are ignored and every stored edge counts, as in the reference.

Not ported: the reference module's ``__getattr__``, which forwards every unknown name to ``networkx.algorithms.centrality`` on a
Python copy of the graph.  This package has no networkx dependency and no CPU path, so an unknown name is an ``AttributeError``.
"""
from __future__ import annotations

from collections import defaultdict

import torch

from .. import _dispatch
from .temporal import temporal_betweenness_centrality, temporal_closeness_centrality, temporal_shortest_paths  # noqa: F401


def _node_ids(graph) -> list:
    """ID of every node index, in index order (tuples for a higher-order layer)."""
    return [graph.mapping.to_id(i) for i in range(graph.n)]


def path_node_traversals(paths) -> dict:
    """Number of times any path traverses each node (reference src/pathpyG/algorithms/centrality.py:52-59): ``{node id: count}`` for
    the nodes that occur, in index order.  Counted on the device the ``PathData`` lives on, read back once."""
    seq = paths.data.node_sequence.reshape(-1)
    if seq.numel() == 0:
        return {}
    if seq.is_cuda:
        from .. import _hip
        bins = paths.mapping.num_ids() if paths.mapping.has_ids else int(seq.max()) + 1
        counts = _hip.degree(seq.to(torch.int64), bins)
    else:
        counts = torch.bincount(seq)
    return {paths.mapping.to_id(i): c for i, c in enumerate(counts.tolist()) if c > 0}


def map_to_nodes(graph, centralities: dict) -> dict:
    """Map a ``{node index: value}`` dictionary to node IDs (reference centrality.py:62-80)."""
    return {graph.mapping.to_id(idx): value for idx, value in centralities.items()}


def source_indices(graph, sources) -> list | None:
    """Node indices of a list of source IDs, in the given order (repeats kept); ``None`` stands for every node.  An unknown ID
    raises what ``graph.mapping.to_idx`` raises."""
    if sources is None:
        return None
    return [int(graph.mapping.to_idx(s)) for s in sources]


def betweenness_centrality(graph, sources: list | None = None) -> dict:
    """Betweenness centrality by Brandes' algorithm, exactly as the reference computes it (centrality.py:83-134).

    ``sources`` lists the node IDs whose shortest-path trees are counted, processed as given (a repeated ID counts twice); default:
    every node.  Returns a ``defaultdict`` (default 0.0) with a key for exactly the nodes that some source reached at distance >= 1,
    zero values included — the reference creates ``bw[w]`` when it first adds ``delta[w]``.  The value follows the reference's
    accumulation, which adds ``delta[w]`` once per predecessor EDGE of ``w`` (its statement sits inside the loop over ``P[w]``):
    a source contributes ``npred[w] * delta[w]``.  networkx's unnormalised betweenness is a different number on most graphs.

    Every source's search runs on the GPU, level-synchronous: path counts ``sigma`` are integer-valued float64 where the reference's
    Python ints are unbounded, and dependencies are pulled in CSR order without floating-point atomics.  While every count of a
    searched source stays below 2**53 the counts are exact, the result has the same bits on every run and equals the reference up to
    float64 summation order.  Between 2**53 and 2**1024 the counts round as they are added, in an order that may differ from run to
    run: the result stays within summation rounding of the reference, its last bits are not reproducible.  A count of 2**1024 or
    more does not fit a float64: the call raises ``OverflowError`` if some node has that many shortest paths from one of the searched
    sources (other sources of the same graph are served).  O(n m) work for all sources.
    """
    bw = defaultdict(lambda: 0.0)
    idx = source_indices(graph, sources)
    n = graph.n
    if n == 0 or (idx is not None and len(idx) == 0):
        return bw
    if idx is not None and (min(idx) < 0 or max(idx) >= n):
        raise IndexError(f"source node index out of range [0, {n})")
    values, reached = _dispatch.graph_betweenness(graph, idx)
    values, reached = values.tolist(), reached.tolist()
    for i in range(n):
        if reached[i]:
            bw[graph.mapping.to_id(i)] = float(values[i])
    return bw


def closeness_from_totals(reach_in, dist_in, n: int) -> list:
    """networkx's ``closeness_centrality`` (incoming distances, Wasserman-Faust factor) from the per-node totals, in float64 and in
    networkx's order of operations: ``(r / tot) * (r / (n - 1))``; 0.0 where no other node reaches the node."""
    out = []
    for r, tot in zip(reach_in, dist_in):
        if tot == 0 or n == 1:
            out.append(0.0)
        else:
            out.append((float(r) / float(tot)) * (float(r) / float(n - 1)))
    return out


def closeness_centrality(graph) -> dict:
    """Closeness centrality as the reference returns it (centrality.py:327-356 delegates to ``networkx.closeness_centrality``):
    for node ``v`` with ``r`` other nodes that reach it over a total distance ``tot``, ``(r / tot) * (r / (n - 1))`` — incoming
    distances, scaled by the reachable fraction (Wasserman and Faust) — and 0.0 if nothing reaches it.  Keys are all node IDs.
    The totals come from the device (``pp_graph_bfs``); no distance matrix is built."""
    n = graph.n
    ids = _node_ids(graph)
    if n <= 1:
        return {i: 0.0 for i in ids}
    reach_in, dist_in, _ = _dispatch.graph_path_totals(graph)
    return dict(zip(ids, closeness_from_totals(reach_in, dist_in, n)))


def path_visitation_probabilities(paths) -> dict:
    """Probability that a randomly chosen node visit of the path data falls on each node (reference centrality.py:137-161): the
    traversal counts of :func:`path_node_traversals` divided by their sum."""
    counts = path_node_traversals(paths)
    total = float(sum(counts.values()))             # integer counts: exact in any order
    return {node: count / total for node, count in counts.items()}
