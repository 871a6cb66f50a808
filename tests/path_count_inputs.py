"""Inputs shared by tests/test_path_counts_host.py, tests/test_gpu_path_counts.py and tests/test_gpu_temporal_paths.py (numpy only, no
product import): structures whose shortest-path counts leave the exact float64 range, and the random streams and component graphs that
make the 1 GiB workspace budget, not the source count or the 2048 / 1024 cap, set a search kernel's grid.

* ``chain(L)``: L stages of two parallel stored edges i -> i+1.  Node k has 2**k shortest paths from node 0: the count reaches 2**1024,
  the first value a float64 cannot hold, at L = 1024.  ``chain_stream(L)`` is the same chain as events: stage i at the times 10 i and
  10 i + 1, so with delta = 11 both events of a stage continue into both events of the next (gaps 9, 10, 10, 11) and into nothing later
  (gap >= 19).
* ``layered()``: 71 layers of 4 nodes, every node sends 2 to 4 edges to distinct nodes of the next layer: irregular counts, no power of two,
  far above 2**53.  ``layered_stream()`` gives the edges of layer l the times 10 l + {0..4}; with delta = 14 an event continues into every
  event of the next layer out of its head (gaps 6 .. 14) and into no later one (gap >= 16): the same path counts as the static graph.
"""
from __future__ import annotations

import numpy as np

CHAIN_DELTA = 11
LAYERED_DELTA = 14
BUDGET = 1 << 30                                  # bytes of per-workgroup search state every search kernel allows itself


def chain(L: int):
    """(edge_index [2, 2 L], n = L + 1)."""
    tail = np.repeat(np.arange(L, dtype=np.int64), 2)
    return np.stack([tail, tail + 1]), L + 1


def chain_stream(L: int):
    """(edge_index [2, 2 L], time [2 L] ascending, n = L + 1); use with ``CHAIN_DELTA``."""
    ei, n = chain(L)
    time = 10 * ei[0] + np.tile(np.array([0, 1], dtype=np.int64), L)
    return ei, time, n


def layered(seed: int = 5, layers: int = 71, width: int = 4):
    """(edge_index [2, m] grouped by layer, n, rng): the generator is handed on so that the stream draws its times from the same sequence."""
    rng = np.random.default_rng(seed)
    tails, heads = [], []
    for layer in range(layers - 1):
        for i in range(width):
            fan = int(rng.integers(2, width + 1))
            for j in rng.choice(width, size=fan, replace=False):
                tails.append(layer * width + i)
                heads.append((layer + 1) * width + int(j))
    return np.array([tails, heads], dtype=np.int64), layers * width, rng


def layered_stream(seed: int = 5, layers: int = 71, width: int = 4):
    """(edge_index [2, m], time [m], n), stably sorted by time; use with ``LAYERED_DELTA``."""
    ei, n, rng = layered(seed, layers, width)
    time = 10 * (ei[0] // width) + rng.integers(0, 5, ei.shape[1])
    order = np.argsort(time, kind="stable")
    return ei[:, order], time[order], n


def exact_counts(edge_index, n: int, s: int) -> list:
    """Number of shortest paths from ``s`` to every node as Python ints (0 = unreachable), every stored edge counted once."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    out = [[] for _ in range(n)]
    for v, w in ei.T.tolist():
        out[v].append(w)
    dist, sigma = [-1] * n, [0] * n
    dist[s], sigma[s] = 0, 1
    frontier = [s]
    while frontier:
        nxt = []
        for v in frontier:
            for w in out[v]:
                if dist[w] < 0:
                    dist[w] = dist[v] + 1
                    nxt.append(w)
                if dist[w] == dist[v] + 1:
                    sigma[w] += sigma[v]
        frontier = nxt
    return sigma


def random_stream(seed: int, n: int, m: int, span: int):
    """(edge_index [2, m], time [m] ascending): uniform endpoints, uniform integer times in [0, span)."""
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, n, (2, m))
    return ei, np.sort(rng.integers(0, span, m))


# The two budget streams: (seed, n, m, span, delta) and the grid the kernels' formulas give for them.
BFS_BUDGET_STREAM = (23, 2100, 45_000, 100_000, 3000)
BFS_BUDGET_SLICES = BUDGET // (12 * 45_000)                       # 1988: below the cap of 2048 and below n = 2100
BETWEENNESS_BUDGET_STREAM = (29, 1100, 30_000, 100_000, 2500)


def up256(x: int) -> int:
    return (x + 255) // 256 * 256


def temporal_betweenness_parts(m: int, n: int) -> int:
    """k_temporal_betweenness' grid: two int32 and three float64 per event, the level starts, an int32 and a float64 per node, each
    piece rounded up to 256 bytes, as many slices as 1 GiB holds, at most n and 1024."""
    block = 2 * up256(4 * m) + up256(4 * (m + 2)) + 3 * up256(8 * m) + up256(4 * n) + up256(8 * n)
    return max(1, min(BUDGET // block, n, 1024))


def graph_betweenness_parts(n: int, n_sources: int) -> int:
    """k_graph_betweenness' grid: three int32 and two float64 per node, the level starts, and the workgroup's float64 row of the result."""
    block = 3 * up256(4 * n) + up256(4 * (n + 2)) + 2 * up256(8 * n) + 8 * n
    return max(1, min(BUDGET // block, n_sources, 1024))


COMPONENT = 8                                     # nodes of one component of ``component_paths``


def component_edges():
    """One component, 8 nodes and 8 edges: the diamond 0 -> {1, 2} -> 3 and the directed path 3 -> 4 -> ... -> 7.  From node 0 the node 3 has
    two tight predecessors and the nodes 3 .. 7 have two shortest paths each; from every other node all counts are 1."""
    tail = np.array([0, 0, 1, 2, 3, 4, 5, 6], dtype=np.int64)
    head = np.array([1, 2, 3, 3, 4, 5, 6, 7], dtype=np.int64)
    return np.stack([tail, head])


def component_paths(n: int, seed: int):
    """(edge_index [2, n], perm [n]): n / 8 disjoint copies of ``component_edges``, node ids carried through a seeded permutation:
    local node j of component c is ``perm[8 c + j]``.  Which of the two tight predecessors of a component's node 3 has the larger index,
    and with it the predecessor the search reports, is decided by the permutation."""
    assert n % COMPONENT == 0
    perm = np.random.default_rng(seed).permutation(n).astype(np.int64)
    local = component_edges()
    base = (np.arange(n // COMPONENT, dtype=np.int64) * COMPONENT)[:, None]
    tail = perm[(base + local[0][None, :]).reshape(-1)]
    head = perm[(base + local[1][None, :]).reshape(-1)]
    return np.stack([tail, head]), perm
