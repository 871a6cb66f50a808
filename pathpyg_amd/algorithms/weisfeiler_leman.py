"""Weisfeiler-Leman isomorphism test and colour refinement (reference src/pathpyG/algorithms/weisfeiler_leman.py:8-75).

The reference adds the two graphs, then builds in every round one Python string per node — ``str(own label) + str(sorted labels of
successors())`` — and numbers the strings through a dict.  Here a round is a CSR gather of successor colours and an exact grouping of the
rows by multiset on the device (``pp_graph_wl_refine``, csrc/pp_graph_wl.hip); :func:`color_refinement` gives that to any
:class:`~pathpyg_amd.core.graph.Graph`, and :func:`WeisfeilerLeman_test` is it on the disjoint union of two graphs, with the reference's
numbering and stop rule computed from the class counts of the rounds.

What the reference's function does, quirks included, and what is kept:

* A node's signature is (own colour, multiset of the colours of its *stored* successors): parallel edges count with their multiplicity, a
  self-loop contributes the node's own colour, predecessors play no part.
* The union's nodes are ordered by ``np.unique`` of the concatenated IDs (``Graph.__add__``); the IDs of the two graphs may interleave.
  Within a round the classes are numbered by first occurrence in that order, and the numbers continue from round to round: round r's
  labels are ``1 + k_1 + ... + k_(r-1) + rank of the class``, k_i the number of classes of round i.
* The loop stops when a round produces as many classes as its input had, and returns the INPUT of that round: regular graphs come back as
  lists of the string ``'0'``, featured ones possibly as the feature values themselves, everything else as Python ints.
* Features are used only if both dicts are given.  The own label enters the string through ``str()``: a string feature ``'1'`` on a node
  without successors gives ``"1[]"``, which a later round produces for the integer colour 1, and the dict then reuses the number.  So the
  device takes features only when the dicts cover exactly the nodes, every value is a ``str`` and none is the decimal form of a positive
  integer; any other pair of dicts runs :func:`_host_test`, the reference's rounds restated literally (same results, same ``KeyError`` /
  ``TypeError``), which is there for completeness, like ``katz_index`` in :mod:`pathpyg_amd.statistics`.

On the host stay: the ``np.unique`` order of the IDs (handed to the device as a rank per node), the overlap check made from the same
``np.unique``, and the mapping of string features to integer codes.  The number of rounds can reach n / 2 (a path); each round is a fixed
number of launches and one read-back, so long thin graphs are bound by launches, as the strong-components search is.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _dispatch
from ..core.graph import Graph

NATIVE = True                       # False: WeisfeilerLeman_test runs the host loop (_host_test) for every input
HASH_MASK = 0xFFFFFFFFFFFFFFFF      # ANDed with the row hashes that speed up grouping; any value, 0 included, gives the same classes
last_stats = None                   # _hip.WlStats (counts, passes per round) of the most recent device run of this module


def color_refinement(graph: Graph, initial: Optional[torch.Tensor] = None, max_rounds: Optional[int] = None,
                     order: Optional[torch.Tensor] = None, with_stats: bool = False):
    """Colour refinement (1-dimensional Weisfeiler-Leman) of any graph: a window, a static aggregate, a higher-order layer.  No ID is touched.

    Args:
        graph: The graph; its stored successor lists are read (parallel edges with multiplicity, self-loops as the own colour).
        initial: int64 ``[n]`` initial colours (any values), or ``None`` for all nodes equal.
        max_rounds: ``None`` refines until the class count stops growing and returns the stable partition; ``h`` returns the partition
            after exactly ``min(h, rounds to stability)`` rounds.
        order: int64 ``[n]``, a permutation: the rank of every node.  Classes are numbered by their first member in this order
            (default: index order).
        with_stats: also return the verify passes of every round (``passes[r]``; one per round unless row hashes collide).

    Returns:
        ``(colors, counts)``: ``colors`` int64 ``[n]`` on the compute device with values 0 .. k-1; ``counts[r]`` the number of classes after
        round r, ``counts[0]`` the number of distinct initial colours.  An unbounded call ends with the round that did not grow the count.
    """
    global last_stats
    colours, stats = _dispatch.graph_color_refinement(graph, _vector(initial, graph.n, "initial"), _vector(order, graph.n, "order"), max_rounds,
                                                     HASH_MASK)
    last_stats = stats
    return (colours, stats.counts, stats.passes) if with_stats else (colours, stats.counts)


def _vector(t, n: int, name: str):
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.dtype != torch.int64 or t.numel() != n:
        raise ValueError(f"{name} must be an int64 vector with one entry per node ({n}), got {t.dtype} with {t.numel()}")
    return t.reshape(-1)


def _ids(g) -> np.ndarray:
    """The IDs of a graph's nodes in index order, as ``Graph.__add__`` reads them (a 2-D array for tuple IDs)."""
    return np.asarray(g.mapping.to_ids(np.arange(g.n)))


def _as_nodes(ids: np.ndarray) -> list:
    """``Graph.nodes`` of the reference: Python scalars, tuples for higher-order nodes."""
    return [tuple(x) for x in ids.tolist()] if ids.ndim > 1 else ids.tolist()


def _device_features(features: dict, nodes: list) -> bool:
    """The rule of the module docstring: may the device take these (merged) features as initial colours?"""
    if len(features) != len(nodes):
        return False
    try:
        if any(v not in features for v in nodes):
            return False
    except TypeError:                                                   # an unhashable node: the host loop raises what the reference raises
        return False
    for f in features.values():
        if type(f) is not str:
            return False
        if f.isascii() and f.isdigit() and f[0] != "0":                 # str(int(f)) == f and int(f) > 0: a later round's own-colour prefix
            return False
    return True


def _host_test(nodes: list, successors: dict, nodes1: list, nodes2: list, features_g1, features_g2):
    """The reference's rounds restated on the union's node list and successor lists (weisfeiler_leman.py:35-75): one string per node and
    round, ``str(own label) + str(sorted successor labels)``, numbered through a dict that lives across the rounds."""
    if features_g1 is None or features_g2 is None:
        current = dict.fromkeys(nodes, "0")
    else:
        current = {**features_g1, **features_g2}
    numbers: dict = {}
    while True:
        refined = {}
        for v in nodes:
            around = [current[w] for w in successors[v]]
            around.sort()
            refined[v] = numbers.setdefault(str(current[v]) + str(around), len(numbers) + 1)
        if len(set(current.values())) == len(set(refined.values())):
            break                                                       # the INPUT of this round is the result
        current = refined
    fp1, fp2 = [current[v] for v in nodes1], [current[v] for v in nodes2]
    return sorted(fp1) == sorted(fp2), fp1, fp2


def _successor_lists(g, nodes: list) -> dict:
    """``{node: successors in stored order}`` from one copy of the (row-sorted) edge list to the host; no device is touched."""
    lists: dict = {v: [] for v in nodes}
    src, dst = g.data.edge_index.cpu().tolist()
    for u, w in zip(src, dst):
        lists[nodes[u]].append(nodes[w])
    return lists


def WeisfeilerLeman_test(g1: Graph, g2: Graph, features_g1: dict | None = None,
                         features_g2: dict | None = None) -> Tuple[bool, List, List]:
    """Run the Weisfeiler-Leman isomorphism test on two graphs.

    ``False`` proves that the graphs are not isomorphic; ``True`` means that no evidence against it was found.  The two graphs must carry
    IndexMaps with disjoint node IDs.

    Args:
        g1: First graph.
        g2: Second graph.
        features_g1: Optional initial node features for graph 1 (``{node ID: value}``).
        features_g2: Optional initial node features for graph 2; features are used only if both are given.

    Returns:
        ``(result, fingerprint_1, fingerprint_2)``, the fingerprints in ``g1.nodes`` and ``g2.nodes`` order with the reference's labels
        (see the module docstring): the string ``'0'``, the feature values, or Python ints.
    """
    global last_stats
    if g1.mapping is None or g2.mapping is None or g1.mapping.node_ids is None or g2.mapping.node_ids is None:
        raise Exception("Graphs must contain IndexMap that assigns node IDs")
    ids1, ids2 = _ids(g1), _ids(g2)
    n1, n2 = len(ids1), len(ids2)
    merged = np.concatenate([ids1, ids2]) if n1 and n2 else (ids1 if n1 else ids2)      # (IDs of different orders: numpy's ValueError, as in g1 + g2)
    rows = merged.ndim > 1
    uniq, rank = np.unique(merged, axis=0 if rows else None, return_inverse=True)
    if len(uniq) != n1 + n2:
        raise Exception("node identifiers of graphs must not overlap")
    rank = np.asarray(rank).reshape(-1)
    nodes1, nodes2 = _as_nodes(ids1), _as_nodes(ids2)

    featured = features_g1 is not None and features_g2 is not None
    merged_features = None
    if featured:
        merged_features = features_g1.copy()
        merged_features.update(features_g2)
    if not NATIVE or (featured and not _device_features(merged_features, nodes1 + nodes2)):
        successors = _successor_lists(g1, nodes1)
        successors.update(_successor_lists(g2, nodes2))
        return _host_test(_as_nodes(uniq), successors, nodes1, nodes2, features_g1, features_g2)

    initial = None
    if featured:
        codes: dict = {}
        initial = torch.tensor([codes.setdefault(merged_features[v], len(codes)) for v in nodes1 + nodes2], dtype=torch.int64)
    colours, stats = _dispatch.graph_pair_color_refinement(g1, g2, initial, torch.from_numpy(rank.astype(np.int64)), HASH_MASK)
    last_stats = stats
    counts = stats.counts
    rounds = len(counts) - 1                                            # the last one is the round that did not grow the count
    if rounds <= 1:                                                     # the input of round 1: the initial fingerprint
        fingerprint = [merged_features[v] for v in nodes1 + nodes2] if featured else ["0"] * (n1 + n2)
    else:                                                               # the output of round `rounds - 1`, numbered after rounds 1 .. rounds - 2
        offset = 1 + sum(counts[1:rounds - 1])
        fingerprint = [offset + c for c in colours.cpu().tolist()]
    fingerprint_1, fingerprint_2 = fingerprint[:n1], fingerprint[n1:]
    return sorted(fingerprint_1) == sorted(fingerprint_2), fingerprint_1, fingerprint_2
