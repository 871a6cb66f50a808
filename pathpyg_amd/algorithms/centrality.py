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

The reference module's ``__getattr__`` forwards every unknown name to ``networkx.algorithms.centrality`` on a Python copy of the graph.
Two of the measures behind that forwarding are native here: :func:`eigenvector_centrality` and :func:`katz_centrality` run networkx's
power iterations as pull products over the predecessor lists of the distinct edges, convergence test included, on the GPU
(``pp_graph_power_iterate``, csrc/pp_graph_power.hip).  ``networkx.pagerank`` is not behind that forwarding (it is link analysis, not
``networkx.algorithms.centrality``): PageRank lives in :mod:`pathpyg_amd.algorithms.ranking`.  The forwarding itself is not ported: this package has no networkx dependency and
no CPU path, so every other forwarded name — ``degree_centrality`` included — is an ``AttributeError``.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np
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


class PowerIterationFailedConvergence(RuntimeError):
    """A power iteration did not meet its criterion within ``max_iter`` iterations (networkx's exception of the same name; this package
    does not depend on networkx, so the class is its own)."""

    def __init__(self, max_iter: int, columns: list | None = None):
        self.max_iter = int(max_iter)
        self.columns = None if columns is None else [int(c) for c in columns]       # a batch: the columns that did not converge
        super().__init__(f"power iteration failed to converge within {self.max_iter} iterations"
                         + ("" if columns is None else f" in columns {self.columns}"))


def _node_vector(value, n: int, name: str) -> torch.Tensor:
    """``value`` (a 1-D tensor or ndarray of length ``n`` in index order, or a dict keyed by node INDEX — the reference's form: its networkx
    copy is index-keyed) as a float64 ``[n]`` tensor on the device it came from."""
    if isinstance(value, dict):
        missing = [i for i in range(n) if i not in value]
        if missing or len(value) != n:
            raise ValueError(f"{name} must have a value for every node index 0 .. {n - 1} and no other key"
                             + (f" (node index {missing[0]} is missing)" if missing else ""))
        return torch.tensor([float(value[i]) for i in range(n)], dtype=torch.float64)
    if isinstance(value, (np.ndarray, list, tuple)):
        value = torch.as_tensor(np.asarray(value, dtype=np.float64))
    if not isinstance(value, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, an ndarray or a dict keyed by node index, got {type(value).__name__}")
    if value.dim() != 1 or value.numel() != n:
        raise ValueError(f"{name} must be a vector with one entry per node ({n}), got shape {tuple(value.shape)}")
    return value.to(torch.float64)


def _check_power_arguments(graph, max_iter: int, weight) -> None:
    if int(max_iter) < 1:
        raise ValueError(f"max_iter must be >= 1, got {max_iter}")
    if weight is not None:
        if weight not in graph.edge_attrs():
            raise KeyError(f"the graph has no edge attribute {weight!r} (it has {graph.edge_attrs()})")
        shape, m = tuple(np.shape(graph.data[weight])), graph.data.edge_index.size(1)
        if len(shape) < 1 or shape[0] != m or int(np.prod(shape)) != m:
            raise ValueError(f"edge attribute {weight!r} must hold one number per stored edge ({m}), got shape {shape}")


def _power_result(graph, values: torch.Tensor, converged: bool, max_iter: int, return_tensor: bool):
    if not converged:
        raise PowerIterationFailedConvergence(max_iter)
    return values if return_tensor else dict(zip(_node_ids(graph), values.tolist()))


def eigenvector_centrality(graph, max_iter: int = 100, tol: float = 1e-06, nstart=None, weight: str | None = None, *,
                           return_tensor: bool = False):
    """Eigenvector centrality as the reference returns it (centrality.py:327-356 forwards to ``networkx.eigenvector_centrality`` on a
    DiGraph copy): the left eigenvector by power iteration with ``A + I`` over the DISTINCT stored edges — parallel edges collapse,
    self-loops stay, the undirected flag plays no part.  From ``x = nstart / sum(nstart)`` (default: all ones) every iteration computes
    ``y[v] = x[v] + sum_{u in pred(v)} w(u, v) x[u]``, divides by ``sqrt(sum y^2)`` (by 1 if that is 0) and stops at the first iterate
    whose L1 distance to the previous one is below ``n * tol``; networkx's arguments, order and defaults.

    ``nstart``: a 1-D tensor or ndarray of length ``n`` in index order, or a dict keyed by node INDEX (the reference's form).  Results are
    pinned for non-negative values; any other vector still ends by ``max_iter``.  ``weight=None`` is the reference.  A string ``weight``
    names an edge attribute of the graph (``"edge_weight"``): an entry's weight is the float64 sum of the attribute over its parallel edges
    — an extension: the reference's copy carries no attributes, so there every ``weight=`` silently reads 1.

    Returns ``{node id: float}`` for all nodes in index order (one read-back), or with ``return_tensor=True`` the float64 ``[n]`` tensor on
    the compute device.  Raises ``ValueError`` for the null graph, an all-zero ``nstart``, a vector of the wrong length or a dict that lacks
    a node, ``KeyError`` for an unknown attribute, :class:`PowerIterationFailedConvergence` after ``max_iter`` iterations without
    convergence.  Everything runs on the GPU (csrc/pp_graph_power.hip); the result has the same bits on every run."""
    n = graph.n
    if n == 0:
        raise ValueError("cannot compute centrality for the null graph")
    _check_power_arguments(graph, max_iter, weight)
    start = None
    if nstart is not None:
        start = _node_vector(nstart, n, "nstart")
        if bool((start == 0).all()):
            raise ValueError("initial vector cannot have all zero values")
    values, _, converged = _dispatch.graph_power_centrality(graph, _dispatch.POWER_EIGENVECTOR, n * tol, int(max_iter), start=start,
                                                     weight=weight)
    return _power_result(graph, values, converged, max_iter, return_tensor)


def katz_centrality(graph, alpha: float = 0.1, beta=1.0, max_iter: int = 1000, tol: float = 1e-06, nstart=None, normalized: bool = True,
                    weight: str | None = None, *, return_tensor: bool = False):
    """Katz centrality as the reference returns it (centrality.py:327-356 forwards to ``networkx.katz_centrality`` on a DiGraph copy):
    from ``x = nstart`` (default: zeros) every iteration computes ``x'[v] = alpha * sum_{u in pred(v)} w(u, v) x[u] + beta[v]`` over the
    DISTINCT stored edges and stops at the first iterate with ``sum |x' - x| < n * tol``; the result is ``x' / sqrt(sum x'^2)`` if
    ``normalized`` (and that norm is not 0), else ``x'``.  networkx's arguments, order and defaults.

    ``beta``: a number for every node, or one value per node; it and ``nstart`` take the forms :func:`eigenvector_centrality` describes,
    and ``weight`` means the same (a named attribute is an extension; ``None`` is the reference).  ``alpha`` at or beyond the reciprocal
    of the largest eigenvalue diverges: the values overflow, the error becomes NaN, which is not below the threshold, and the call raises
    after ``max_iter`` iterations.

    Returns ``{node id: float}`` in index order or, with ``return_tensor=True``, the float64 ``[n]`` tensor on the compute device.  For the null
    graph nothing is computed: ``{}``, or an empty float64 tensor on the device the graph lives on (the host for a CPU-resident graph).
    Raises as :func:`eigenvector_centrality` does (no all-zero refusal: zeros are the default start)."""
    n = graph.n
    _check_power_arguments(graph, max_iter, weight)
    if n == 0:
        return torch.empty(0, dtype=torch.float64, device=graph.device) if return_tensor else {}
    b = float(beta) if isinstance(beta, (int, float, np.integer, np.floating)) else _node_vector(beta, n, "beta")
    start = None if nstart is None else _node_vector(nstart, n, "nstart")
    values, _, converged = _dispatch.graph_power_centrality(graph, _dispatch.POWER_KATZ, n * tol, int(max_iter), alpha=float(alpha),
                                                     beta=b, start=start, normalized=bool(normalized), weight=weight)
    return _power_result(graph, values, converged, max_iter, return_tensor)
