"""Degree statistics of a :class:`~pathpyg_amd.core.graph.Graph` (reference src/pathpyG/statistics/degrees.py:9-326).

Degree vectors are the device-counted ``Graph.degrees(..., return_tensor=True)``; the histogram behind the distribution is ``bincount`` as a
kernel (``pp_degree_i64`` on the degree sequence).  The distribution is returned on the graph's device.  The moments and the generating function
copy that short histogram (``max degree + 1`` entries) to the host and evaluate the reference's float32 torch expressions there: on a CUDA
graph the reference's own code mixes devices and raises, so the CPU evaluation is the only behaviour there is to match.

Two functions work on exact integers where the reference rounds, which is a documented deviation at scale:

* ``degree_assortativity`` takes ``S_1, S_2, S_3`` (from the histogram, Python ints) and ``S_e`` (``pp_degree_product_sum``, int64) exactly
  and evaluates the reference's closing expression in Python floats.  The reference accumulates all four in float32: it equals this
  function whenever every one of its sums is exact (all below 2**24) and drifts beyond.
* ``mean_neighbor_degree`` forms its products in int64; the reference's int32 product wraps for degrees above 46 340.
"""
from __future__ import annotations

import numpy as _np
import torch

from .. import _dispatch
from ..core.graph import Graph


def degree_sequence(graph: Graph, mode: str = "total") -> torch.Tensor:
    """The (unweighted) degree of every node, in index order: int32 ``[n]`` on the graph's device.

    Args:
        graph: The graph.
        mode: ``"in"``, ``"out"`` or ``"total"`` (in + out); a graph flagged undirected has its in-degrees as ``"total"``.
    """
    if mode != "total":
        return graph.degrees(mode, return_tensor=True)
    inward = graph.degrees(mode="in", return_tensor=True)
    if graph.is_undirected():
        return inward
    return inward + graph.degrees(mode="out", return_tensor=True)


def _histogram(graph: Graph, mode: str) -> torch.Tensor:
    """Number of nodes per degree, int32 ``[max degree + 1]`` on the compute device (empty for a graph without nodes)."""
    return _dispatch.degree_histogram(graph, degree_sequence(graph, mode=mode))


def _power_sums(histogram: torch.Tensor, powers) -> list:
    """``sum_i d_i**p`` for every ``p`` as exact Python ints, from the degrees that occur."""
    counts = histogram.cpu().numpy()
    occurring = _np.nonzero(counts)[0]
    pairs = list(zip(occurring.tolist(), counts[occurring].tolist()))
    return [sum(c * d ** p for d, c in pairs) for p in powers]


def degree_distribution(graph: Graph, mode: str = "total") -> torch.Tensor:
    """The fraction of nodes per degree ``0 .. max degree``: float32 ``[max degree + 1]`` on the graph's device.  The short histogram is
    divided by ``n`` on the host, where the quotient is correctly rounded as in the reference; dividing a device tensor by a scalar
    multiplies by the rounded reciprocal, which is off by an ulp for some counts (7 / 12)."""
    return (_histogram(graph, mode).cpu() / graph.n).to(graph.device)


def _host_distribution(graph: Graph, mode: str):
    p_k = degree_distribution(graph, mode=mode).cpu()
    return p_k, torch.arange(len(p_k), dtype=torch.float32)


def degree_raw_moment(graph: Graph, k: int = 1, mode: str = "total") -> float:
    """The k-th raw moment ``sum_d d**k P(d)`` of the degree distribution, in float32 on the host."""
    p_k, d = _host_distribution(graph, mode)
    return torch.sum(d.pow(k) * p_k).item()


def mean_degree(graph: Graph, mode: str = "total") -> float:
    """The mean degree, as float32 (the reference's ``torch.mean`` of the float32 sequence): the exact integer sum of the degrees, rounded
    once and divided by ``n``.  It equals the reference whenever its float32 sum is exact (below 2**24); ``nan`` without nodes."""
    total = _power_sums(_histogram(graph, mode), (1,))[0]
    return (torch.tensor(float(total), dtype=torch.float32) / graph.n).item()


def mean_neighbor_degree(graph: Graph, mode: str = "total", exclude_backlink: bool = False) -> float:
    """The mean degree of a neighbour: ``sum_v d_in(v) d_mode(v)`` over the number of edges (twice that for an undirected graph), with
    ``d_mode - 1`` under ``exclude_backlink``.  The sum is taken over the stored edges as ``sum_e d_mode(dst(e))``, an exact integer."""
    total = _dispatch.degree_product_sum(graph, None, degree_sequence(graph, mode=mode))
    if exclude_backlink:
        total -= int(graph.data.edge_index.size(1))                     # sum_v d_in(v)
    return total / (2 * graph.m if graph.is_undirected() else graph.m)


def degree_central_moment(graph: Graph, k: int = 1, mode: str = "total") -> float:
    """The k-th central moment ``sum_d (d - <d>)**k P(d)`` of the degree distribution (k = 2: its variance), in float32 on the host."""
    p_k, d = _host_distribution(graph, mode)
    centre = mean_degree(graph, mode=mode)
    return torch.sum((d - centre).pow(k) * p_k).item()


def degree_assortativity(graph: Graph, mode: str = "total") -> float:
    """The degree assortativity coefficient ``(S_1 S_e - S_2**2) / (S_1 S_3 - S_2**2)`` with ``S_l = sum_i d_i**l`` and
    ``S_e = sum over stored edges of d_i d_j`` (Newman, Networks, 10.27-10.28).  ``ZeroDivisionError`` for a regular or empty graph, as
    in the reference.  See the module text for the exact-integer deviation."""
    seq = degree_sequence(graph, mode=mode)
    s_1, s_2, s_3 = (float(total) for total in _power_sums(_dispatch.degree_histogram(graph, seq), (1, 2, 3)))
    s_e = float(_dispatch.degree_product_sum(graph, seq, seq))
    return (s_1 * s_e - s_2 ** 2) / (s_1 * s_3 - s_2 ** 2)


def degree_generating_function(graph: Graph, x, mode: str = "total"):
    """The probability generating function ``f(x) = sum_d P(d) x**d`` of the degree distribution.

    Args:
        graph: The graph.
        x: A float (a float comes back), or a list, ``numpy.ndarray`` or ``torch.Tensor`` of arguments (a float32 CPU tensor comes back).
        mode: ``"in"``, ``"out"`` or ``"total"``.

    Raises:
        TypeError: for any other type of ``x`` (a Python int among them).
    """
    if isinstance(x, float):                                            # (the argument is judged before the device is touched)
        points = torch.tensor([x])
    elif isinstance(x, (list, _np.ndarray)):
        points = torch.tensor(x, dtype=torch.float32)
    elif isinstance(x, torch.Tensor):
        points = x.detach().cpu().float()
    else:
        raise TypeError("x must be a float, list, numpy.ndarray, or torch.Tensor")
    p_k = degree_distribution(graph, mode=mode).cpu()
    powers = points.unsqueeze(0) ** torch.arange(p_k.size(0)).unsqueeze(1)
    values = torch.sum(p_k.unsqueeze(1) * powers, dim=0)
    return values[0].item() if isinstance(x, float) else values
