"""Similarity measures between two nodes of a :class:`~pathpyg_amd.core.graph.Graph` (reference
src/pathpyG/statistics/node_similarities.py:11-255).

The reference rebuilds two Python sets per pair and, for the cosine similarity, densifies the n x n adjacency matrix.  Here every set-based
measure is the intersection of two sorted successor lists on the device (``pp_graph_pair_meets``, csrc/pp_graph_triads.hip), which returns
three numbers per pair: the common successors, the dot product of the two adjacency rows (parallel edges summed, as the reference's dense
matrix sums them) and the Adamic-Adar sum, whose terms ``1 / log(out-degree)`` are tabulated by numpy on the host — the reference's own
bits, ``inf`` at out-degree 1 included.  The scalar functions run a batch of one pair and finish in Python, with the reference's return
types and exceptions; :func:`pairwise` runs any number of pairs and finishes on the device.

``katz_index`` and ``LeichtHolmeNewman_index`` invert n x n matrices with scipy on the host, as the reference does; they are here so that
the module is complete, not because they are fast.
"""
from __future__ import annotations

import numpy as _np
import torch

from .. import _dispatch, _hip
from ..core.graph import Graph
from .degrees import degree_sequence

_MEASURES = ("common_neighbors", "overlap", "jaccard", "adamic_adar", "cosine")


def _one_pair(graph: Graph, v, w) -> torch.Tensor:
    return torch.tensor([[int(graph.mapping.to_idx(v))], [int(graph.mapping.to_idx(w))]], dtype=torch.int64)


def _adamic_adar_table(graph: Graph) -> _np.ndarray:
    """``1 / log(d)`` for every stored out-degree ``d = 0 .. max``, as numpy evaluates it: ``-0.0`` at 0 and ``inf`` at 1."""
    ptr = graph.row_ptr
    widest = int((ptr[1:] - ptr[:-1]).max().item()) if graph.n else 0
    with _np.errstate(divide="ignore"):
        return 1 / _np.log(_np.arange(widest + 1))


def _meets(graph: Graph, pairs, measure: str):
    """The integers a measure needs for the index pairs ``pairs`` [2, P], on the compute device."""
    table = _adamic_adar_table(graph) if measure == "adamic_adar" else None
    common, dot, aa, sizes = _dispatch.graph_pair_meets(graph, pairs, table, want_dot=measure == "cosine",
                                                        want_sizes=measure in ("overlap", "jaccard"))
    norm2 = None
    if measure == "cosine":                                             # |A_v|^2 and |A_w|^2: every node met with itself
        both = torch.cat((pairs[0], pairs[1]))
        norm2 = _dispatch.graph_pair_meets(graph, torch.stack((both, both)), want_dot=True)[1].reshape(2, -1)
    return common, dot, aa, sizes, norm2


def inverse_path_length(graph: Graph, v, w) -> float:
    """``1 / d(v, w)`` for the shortest-path distance ``d``: ``inf`` for ``v == w`` and 0.0 without a path.  One search from ``v`` on the
    device (``pp_graph_bfs``), not the n x n distance matrix of the reference."""
    target = int(graph.mapping.to_idx(w))
    dist, _ = _dispatch.graph_shortest_paths(graph, [int(graph.mapping.to_idx(v))])
    d = int(dist[0, target].item())
    if d == 0:
        return _np.inf
    return 1 / _np.float64(_np.inf if d < 0 else d)


def common_neighbors(graph: Graph, v, w) -> float:
    """The number of common successors of ``v`` and ``w``."""
    return int(_meets(graph, _one_pair(graph, v, w), "common_neighbors")[0].item())


def overlap_coefficient(graph: Graph, v, w) -> float:
    """Common successors over the smaller of the two successor sets; ``ZeroDivisionError`` when either set is empty."""
    common, _, _, sizes, _ = _meets(graph, _one_pair(graph, v, w), "overlap")
    return int(common.item()) / min(sizes.reshape(-1).tolist())


def jaccard_similarity(graph: Graph, v, w) -> float:
    """Common successors over the union of the two successor sets; the int 1 when both sets are empty."""
    common, _, _, sizes, _ = _meets(graph, _one_pair(graph, v, w), "jaccard")
    n_v, n_w = sizes.reshape(-1).tolist()
    if n_v == 0 and n_w == 0:
        return 1
    shared = int(common.item())
    return shared / (n_v + n_w - shared)


def adamic_adar_index(graph: Graph, v, w) -> float:
    """The sum of ``1 / log(out-degree of u)`` over the common successors ``u`` (Adamic and Adar 2003); ``inf`` as soon as a common
    successor has out-degree 1, the int 0 without common successors."""
    common, _, aa, _, _ = _meets(graph, _one_pair(graph, v, w), "adamic_adar")
    return _np.float64(aa.item()) if int(common.item()) else 0


def cosine_similarity(graph: Graph, v, w) -> float:
    """The cosine of the angle between the adjacency rows of ``v`` and ``w`` (Newman, Networks, 7.35).  As in the reference the int 0 comes
    back when the IN-degree of either node is 0, and ``nan`` when an out-row is empty otherwise."""
    pair = _one_pair(graph, v, w)
    inward = graph.degrees(mode="in", return_tensor=True)
    if int(inward[pair[0, 0]]) == 0 or int(inward[pair[1, 0]]) == 0:
        return 0
    _, dot, _, _, norm2 = _meets(graph, pair, "cosine")
    a, b = norm2.reshape(-1).tolist()
    with _np.errstate(invalid="ignore"):
        return _np.float64(int(dot.item())) / (_np.sqrt(_np.float64(a)) * _np.sqrt(_np.float64(b)))


def pairwise(graph: Graph, pairs, measure: str) -> torch.Tensor:
    """One measure for many node pairs in one device pass.

    Args:
        graph: The graph.
        pairs: An int64 ``[2, P]`` tensor of node indices, or a list of ``(v, w)`` node-ID pairs.
        measure: ``"common_neighbors"``, ``"overlap"``, ``"jaccard"``, ``"adamic_adar"`` or ``"cosine"``.

    Returns:
        float64 ``[P]`` on the graph's device (int64 for ``"common_neighbors"``): the value of the scalar function for every pair, ``nan``
        where the scalar function raises (``"overlap"`` with an empty successor set).
    """
    if measure not in _MEASURES:
        raise ValueError(f"unknown measure {measure!r}: one of {', '.join(_MEASURES)}")
    if isinstance(pairs, torch.Tensor):
        if pairs.dim() != 2 or pairs.size(0) != 2:
            raise ValueError(f"pairs must have shape [2, P], got {tuple(pairs.shape)}")
        pairs = pairs.to(torch.int64)
    else:
        to_idx = graph.mapping.to_idx
        pairs = torch.tensor([[int(to_idx(v)), int(to_idx(w))] for v, w in pairs], dtype=torch.int64).reshape(-1, 2).T.contiguous()
    dev = _dispatch.compute_device(graph.data.edge_index)
    pairs = pairs.to(dev).contiguous()
    common, dot, aa, sizes, norm2 = _meets(graph, pairs, measure)
    if measure == "common_neighbors":
        return _dispatch._back(graph.data.edge_index, common)
    inward = graph.degrees(mode="in", return_tensor=True).to(dev) if measure == "cosine" else None
    out = _hip.pair_measure(measure, graph.n, pairs, common, dot, aa, sizes, norm2, inward)
    return _dispatch._back(graph.data.edge_index, out)


def katz_index(graph: Graph, v, w, beta: float) -> float:
    """The Katz index ``((I - beta A)^-1 - I)[v, w]`` (Katz 1953).  Host code: scipy inverts the n x n matrix, as in the reference."""
    import scipy.sparse as _sparse
    import scipy.sparse.linalg as _linalg

    adj = graph.sparse_adj_matrix()
    eye = _sparse.identity(graph.n)
    s = _linalg.inv(eye - beta * adj) - eye
    return s[graph.mapping.to_idx(v), graph.mapping.to_idx(w)]


def LeichtHolmeNewman_index(graph: Graph, v, w, alpha: float) -> float:  # noqa: N802 - the reference's name
    """The Leicht-Holme-Newman index ``2 m lambda_1 D^-1 (I - alpha A / lambda_1)^-1 D^-1 [v, w]`` (Leicht, Holme and Newman 2006), with
    ``lambda_1`` the largest eigenvalue of the adjacency matrix and ``D`` the diagonal matrix of total degrees.  Host code: scipy computes the
    eigenvalues and inverts three n x n matrices, as in the reference."""
    import scipy.sparse as _sparse
    import scipy.sparse.linalg as _linalg

    adj = graph.sparse_adj_matrix()
    largest = _np.sort(_np.absolute(_linalg.eigs(adj, which="LM", k=2, return_eigenvectors=False)))[1]
    deg_inv = _linalg.inv(_sparse.diags(degree_sequence(graph).cpu().numpy()).tocsc())
    eye = _sparse.identity(graph.n).tocsc()
    s = 2 * graph.m * largest * deg_inv * _linalg.inv(eye - alpha * adj / largest) * deg_inv
    return s[graph.mapping.to_idx(v), graph.mapping.to_idx(w)]
