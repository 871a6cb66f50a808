"""Temporal event-graph lift, HIP-backed (reference ``pathpyG.algorithms.temporal``)."""
from __future__ import annotations

import torch

from .. import _dispatch


def lift_order_temporal(g, delta: float | int = 1) -> torch.Tensor:
    """Lift a temporal graph to its second-order event graph (reference src/pathpyG/algorithms/temporal.py:17-54).

    Returns the int64 ``[2, E2]`` index of all event pairs ``(i, j)`` with ``dst(i) == src(j)`` and
    ``t_i < t_j <= t_i + delta``, in lexicographic order, on the device of ``g.data.edge_index``.
    ``delta`` is interpreted exactly like ``torch.tensor(delta)`` in the reference: an ``int`` compares
    in int64, a Python ``float`` against int64 timestamps compares in float32, ``np.float64`` in float64.

    Differences from the reference, both deliberate: the per-timestamp Python loop is replaced by a
    sort/search/scan/fill pipeline of HIP kernels, and an event list without any admissible pair yields an
    empty ``[2, 0]`` tensor instead of the reference's ``torch.cat([])`` error (temporal.py:53).
    Supported timestamp dtypes: integer types (widened to int64) and float64.
    """
    data = g.data
    return _dispatch.temporal_lift(data.edge_index, data.time, int(data.num_nodes), delta)


def temporal_shortest_paths(g, delta: int):
    """Shortest time-respecting paths between all first-order nodes (reference src/pathpyG/algorithms/temporal.py:57-107).

    Returns ``(dist, pred)`` as numpy arrays like the reference: ``dist[s, v]`` = number of events on a shortest time-respecting
    path (``inf`` if there is none, ``0`` on the diagonal), ``pred[s, v]`` = source node of the last event of such a path (``-1``
    if none, ``s`` on the diagonal).  The reference runs scipy's Dijkstra on an augmented event DAG; here every source node runs a
    frontier BFS on the lifted event graph on the GPU.  Distances are identical; where several events complete a shortest path
    the LATEST one names the predecessor (scipy: whichever its heap pops first) — the reference's known answer is reproduced.
    The result is dense ``n x n``: like the reference this is meant for graphs with thousands, not millions, of nodes.
    """
    import numpy as np

    data = g.data
    dist, pred = _dispatch.temporal_bfs(data.edge_index, data.time, int(data.num_nodes), delta)
    dist = dist.cpu().numpy().astype(np.float64)
    dist[dist < 0] = np.inf
    return dist, pred.cpu().numpy()


def temporal_closeness_centrality(graph, delta: int) -> dict:
    """Temporal closeness centrality (reference src/pathpyG/algorithms/centrality.py:300-326): for every node ``x`` the sum over
    all other nodes ``s`` of ``(n - 1) / dist[s, x]`` with the shortest time-respecting path distances of
    :func:`temporal_shortest_paths` (unreachable pairs contribute 0).  Same summation order as the reference (sources ascending)."""
    import numpy as np

    dist, _ = temporal_shortest_paths(graph, delta)
    n = graph.n
    centralities = {}
    others = np.arange(n)
    for x in graph.nodes:
        i = graph.mapping.to_idx(x)
        centralities[x] = float(sum((n - 1) / dist[others != i, i]))
    return centralities


def temporal_betweenness_centrality(graph, delta: int = 1):
    """Temporal betweenness centrality based on shortest time-respecting paths with maximum waiting time ``delta`` (reference
    src/pathpyG/algorithms/centrality.py:164-297: Brandes' algorithm on the event DAG, pure-Python dict/deque loops per source).

    Here every source node runs the level-synchronous form of the same recurrences on the GPU (``pp_temporal_betweenness``):
    float64 path counts like the reference's, dependencies accumulated in float64 — equal to the reference up to summation order
    (its known answer is reproduced exactly).  While every path count stays below 2**53 the counts are exact and the result has the
    same bits on every run; between 2**53 and 2**1024 the counts round as they are added, in an order that may differ from run to
    run, and the result stays within summation rounding of the reference; from 2**1024 on a count is ``inf`` here as it is there, and
    the backward pass follows the reference's guard (centrality.py:282-289): a ratio ``inf / inf`` counts as 0.0, so the result is
    finite wherever the reference's is.  Returns a ``defaultdict`` node id -> centrality with an entry for every node."""
    from collections import defaultdict

    data = graph.data
    bw = _dispatch.temporal_betweenness(data.edge_index, data.time, int(data.num_nodes), delta).cpu().tolist()
    out = defaultdict(lambda: 0.0)
    for idx, value in enumerate(bw):
        out[graph.mapping.to_id(idx)] = float(value)
    return out
