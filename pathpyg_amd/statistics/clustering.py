"""Closed triads and clustering coefficients of a :class:`~pathpyg_amd.core.graph.Graph` (reference
src/pathpyG/statistics/clustering.py:10-88).

The reference finds the closed triads of ONE node with a doubly nested Python loop over successor lists, and
``avg_clustering_coefficient`` repeats that for every node, building the ``{node: degree}`` dictionary up to three times per node.  Here the
closed triads of all nodes come from one device pass over the graph's simple successor structure (``Graph.simple_successors()``): for every
entry ``(v, x)`` the size of ``S(x) ∩ S(v)`` (csrc/pp_graph_triads.hip), summed per row.  That number is the size of the reference's
``closed_triads(g, v)`` set on any multigraph, self-loops included.  The single-node functions run the same pass on the one row they need and
read one degree from the degree vector; no dictionary is built.

Normalisation, as in the reference: a directed graph divides by ``d (d - 1)`` with ``d`` the STORED out-degree (parallel edges count), a
graph flagged undirected by the same expression of the stored IN-degree (the reference calls ``degrees()`` with its default mode) after
halving and doubling the count; 0.0 where ``d <= 1``.  Every step is exact or one correctly rounded float64 division, so the values equal
the reference's bit for bit.
"""
from __future__ import annotations

from typing import Set

import torch

from .. import _dispatch
from ..core.graph import Graph


def closed_triad_counts(g: Graph) -> torch.Tensor:
    """The number of closed triads around every node, ``len(closed_triads(g, v))`` for all ``v`` at once: int64 ``[n]`` on the graph's device."""
    if g.n == 0:
        return torch.empty(0, dtype=torch.int64, device=g.device)
    return _dispatch._back(g.data.edge_index, _dispatch.graph_triad_counts(g))


def local_clustering_coefficients(g: Graph) -> torch.Tensor:
    """The local clustering coefficient of every node: float64 ``[n]`` on the graph's device, each entry equal to
    ``local_clustering_coefficient(g, node)``."""
    if g.n == 0:
        return torch.empty(0, dtype=torch.float64, device=g.device)
    coeff, _ = _dispatch.graph_clustering(g, _dispatch.graph_triad_counts(g), True, False)
    return _dispatch._back(g.data.edge_index, coeff)


def _degree_of(g: Graph, index: int) -> int:
    return int(g.degrees(mode="in" if g.is_undirected() else "out", return_tensor=True)[index])


def local_clustering_coefficient(g: Graph, u) -> float:
    """Local clustering coefficient of node ``u``: the closed triads around ``u`` over the possible ones.

    Args:
        g: The graph.
        u: The node ID.
    """
    index = int(g.mapping.to_idx(u))
    count, _ = _dispatch.graph_triads_of(g, index, want_pairs=False)
    d = _degree_of(g, index)
    if d <= 1:
        return 0.0
    k = float(count)
    if g.is_directed():
        return k / (d * (d - 1))
    k /= 2.0
    return 2.0 * k / (d * (d - 1))


def avg_clustering_coefficient(g: Graph) -> float:
    """Average of the local clustering coefficients of all nodes (Watts and Strogatz; not the global clustering coefficient).

    As in the reference every local value is rounded to float32 before it is averaged.  The rounded values are summed on the device in
    float64 with a fixed shape and the mean is rounded to float32 once: the same bits on every call, within float32 summation error of the
    reference's ``torch.mean``.  ``nan`` for a graph without nodes (the mean of an empty tensor).
    """
    if g.n == 0:
        return float("nan")
    _, mean = _dispatch.graph_clustering(g, _dispatch.graph_triad_counts(g), False, True)
    return float(mean.item())


def closed_triads(g: Graph, v) -> Set:
    """The set of edges ``(x, y)`` that close a triad around ``v``: ``x`` and ``y`` are successors of ``v`` and ``y`` is a successor of ``x``.
    IDs as the graph's mapping gives them (tuples for a higher-order layer).  Counted, scanned and filled on the device; the pairs travel
    to the host once."""
    index = int(g.mapping.to_idx(v))
    count, pairs = _dispatch.graph_triads_of(g, index, want_pairs=True)
    if count == 0:
        return set()
    xs, ys = pairs.cpu().tolist()
    to_id = g.mapping.to_id
    return {(to_id(x), to_id(y)) for x, y in zip(xs, ys)}
