"""Connected components and the largest connected component of a :class:`~pathpyg_amd.core.graph.Graph` (reference
src/pathpyG/algorithms/components.py:14-53).

The reference copies the edge list to the host, labels it with ``scipy.sparse.csgraph.connected_components`` and filters ``graph.edges``
in a Python loop with two dictionary lookups per edge.  Here the labels, the component sizes, the choice of the largest component and the
filtered, renumbered edge list all come from the device (``pp_graph_components`` and its companions, csrc/pp_graph_components.hip): weak
components by a lock-free union-find over the stored edge list, strong ones by forward colouring and a backward search on the graph's CSR
and CSC.  Only the labels (``connected_components``) or the kept node indices (``largest_connected_component``) travel to the host.

The strong search is level-synchronous: its number of launches grows with the longest shortest path of the graph (a directed ring of k
nodes needs about 2k sweeps); aggregated streams have a small diameter.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import _dispatch, _hip
from ..core.graph import Graph
from ..core.index_map import IndexMap
from ..data import Data


def _strong(graph: Graph, connection) -> bool:
    kind = str(connection).lower()
    if kind not in ("weak", "strong"):
        raise ValueError("connection must be 'weak' or 'strong'")
    # scipy ignores `connection` for directed=False and symmetrises the matrix: an undirected graph has weak components only
    return kind == "strong" and not graph.is_undirected()


def connected_components(graph: Graph, connection="weak") -> Tuple[int, np.ndarray]:
    """Compute the connected components of a graph.

    Args:
        graph: The input graph.
        connection: ``"weak"`` or ``"strong"`` (any letter case).  Ignored for an undirected graph, whose components are the weak ones.

    Returns:
        The number of components and an int32 array with the component label of every node.  Components are numbered in the order of
        their smallest node index.  For weak components that is scipy's own numbering, so the array equals the reference's.  Strong labels
        describe the same partition as the reference's, with the same count, but scipy numbers strong components in the order in which
        Tarjan's search completes them; this numbering is the documented deviation (as the predecessor tie rule of
        ``shortest_paths_dijkstra`` is).
    """
    strong = _strong(graph, connection)
    if graph.n == 0:
        return 0, np.empty(0, dtype=np.int32)
    _, labels, _ = _dispatch.graph_components(graph, strong)
    labels = labels.cpu().numpy()
    return (int(labels.max()) + 1), labels


def _ordered_ids(kept_ids: np.ndarray):
    """The IDs of ``Graph.from_edge_list`` for an edge list over exactly ``kept_ids`` (distinct): ``(node_ids, rank)`` with
    ``node_ids[rank[i]] == kept_ids[i]``.  The rule is ``np.unique``, all-numeric strings in numeric order (core/graph.py)."""
    kept_ids = np.array(kept_ids.tolist())                              # the dtype np.array(edge_list) gives (string width of the kept IDs)
    order = np.argsort(kept_ids, kind="stable")
    node_ids = kept_ids[order]
    if np.issubdtype(node_ids.dtype, np.str_) and np.char.isnumeric(node_ids).all():
        numbers = node_ids.astype(int)
        by_number = np.argsort(numbers, kind="stable")
        order, node_ids = order[by_number], numbers[by_number].astype(str)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    if not np.array_equal(node_ids[rank], kept_ids):                    # "007" -> "7": from_edge_list then fails to look the ID up
        raise KeyError(kept_ids[node_ids[rank] != kept_ids][0])
    return node_ids, rank


def largest_connected_component(graph: Graph, connection="weak") -> Graph:
    """Extract the largest connected component from a graph.

    Args:
        graph: The input graph.
        connection: ``"weak"`` or ``"strong"`` (any letter case); ignored for an undirected graph.

    Returns:
        A new graph with the edges whose two ends lie in the largest component, in their stored order, built as
        ``Graph.from_edge_list(kept edges, is_undirected=graph.is_undirected(), device=graph.device)`` builds it: the kept node IDs,
        indexed in ``from_edge_list``'s order.  Among components of equal largest size the one with the smallest node index is taken
        (the reference's ``Counter(labels).most_common(1)``).  Node and edge attributes are dropped, as in the reference; a largest
        component of one node without a self-loop gives the empty graph.
    """
    strong = _strong(graph, connection)
    device = graph.device

    def assemble(edges) -> Graph:
        return Graph.from_edge_list(edges, is_undirected=graph.is_undirected(), device=device)

    if graph.n == 0:
        return assemble([])
    count, labels, sizes = _dispatch.graph_components(graph, strong)
    keep, size = _hip.graph_components_largest(sizes, count)
    if graph.order > 1:                                                 # tuple IDs: the reference's own expression on the device's labels
        lab = labels.cpu().numpy()
        to_idx = graph.mapping.to_idx
        return assemble([(v, w) for v, w in graph.edges if lab[to_idx(v)] == keep and lab[to_idx(w)] == keep])
    nodes = _hip.graph_component_nodes(labels, keep, size).cpu().numpy()
    kept_ids = np.asarray(graph.mapping.node_ids)[nodes] if graph.mapping.has_ids else nodes
    node_ids, rank = _ordered_ids(kept_ids)
    table = np.full(graph.n, -1, dtype=np.int64)
    table[nodes] = rank
    (ei,) = _dispatch._stage(labels.device, graph.data.edge_index)
    edge_index = _hip.graph_component_edges(ei, labels, keep, torch.from_numpy(table).to(labels.device))
    if edge_index.size(1) == 0:                                         # one node without a self-loop: no edge names it
        return assemble([])
    g = Graph(Data(edge_index=edge_index.to(device), num_nodes=len(node_ids)), mapping=IndexMap(node_ids))
    g.is_undirected_flag = bool(graph.is_undirected())
    return g
