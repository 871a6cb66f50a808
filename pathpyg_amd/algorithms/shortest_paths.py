"""Shortest paths in static graphs, HIP-backed (reference ``pathpyG.algorithms.shortest_paths``).

The reference hands the adjacency matrix to scipy's Dijkstra with ``unweighted=True``; with unit weights that is a breadth-first
search from every node.  Here every node's search runs as a level-synchronous frontier search on the graph's CSR on the GPU
(``pp_graph_bfs``, csrc/pp_graph_paths.hip).  Every function takes any :class:`~pathpyg_amd.core.graph.Graph` — an aggregated
static graph, one window of a ``RollingTimeWindow``, a higher-order layer of a ``MultiOrderModel`` — on any device; edge weights
are ignored and every stored edge counts, as in the reference.  ``directed=graph.is_directed()`` needs no switch: an undirected
``Graph`` stores both directions.
"""
from __future__ import annotations

import numpy as _np

from .. import _dispatch


def shortest_paths_dijkstra(graph) -> tuple[_np.ndarray, _np.ndarray]:
    """All-pairs unit-weight shortest paths (reference src/pathpyG/algorithms/shortest_paths.py:13-24).

    Returns ``(dist, pred)`` as scipy returns them for ``unweighted=True``: ``dist`` float64 ``[n, n]`` with ``inf`` for
    unreachable pairs and a zero diagonal, ``pred`` int32 ``[n, n]`` with ``pred[i, j]`` the node before ``j`` on a shortest
    path from ``i`` and ``-9999`` on the diagonal and for unreachable pairs.  ``dist`` equals scipy's exactly.  Where several
    neighbours of ``j`` lie on shortest paths from ``i`` the one with the LARGEST node index names the predecessor (scipy:
    whichever its heap settles first), so ``pred`` is a valid predecessor matrix that may differ from scipy's on ties.
    This is the only function of the module that builds anything of size ``n x n``.
    """
    n = graph.n
    if n == 0:
        return _np.zeros((0, 0), dtype=_np.float64), _np.zeros((0, 0), dtype=_np.int32)
    dist, pred = _dispatch.graph_shortest_paths(graph)
    dist = dist.cpu().numpy().astype(_np.float64)
    dist[dist < 0] = _np.inf
    return dist, pred.cpu().numpy()


def _scalars(graph) -> tuple[int, int, int]:
    """(sum of the finite off-diagonal distances, largest finite distance, ordered pairs without a path)."""
    _, _, totals = _dispatch.graph_path_totals(graph)
    return int(totals[0]), int(totals[1]), int(totals[2])


def diameter(graph) -> float:
    """Largest shortest-path distance, ``max(dist)`` (reference shortest_paths.py:27-38): ``inf`` as soon as one ordered pair has
    no path.  Computed from per-source totals on the device: no distance matrix is built."""
    if graph.n <= 1:
        return 0.0
    _, longest, no_path = _scalars(graph)
    return float("inf") if no_path else float(longest)


def avg_path_length(graph) -> float:
    """Average shortest-path distance, ``sum(dist) / (n (n - 1))`` (reference shortest_paths.py:41-52): ``inf`` as soon as one
    ordered pair has no path, ``nan`` for a single node (numpy's 0 / 0).  No distance matrix is built."""
    n = graph.n
    if n <= 1:
        return float("nan")
    total, _, no_path = _scalars(graph)
    return float("inf") if no_path else float(_np.float64(total) / (n * (n - 1)))
