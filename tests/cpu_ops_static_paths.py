"""Plain Python / numpy restatement of the static shortest-path and centrality contract (no torch, no GPU), written from the
specification, not from the kernels:

* unit-weight breadth-first search from every source on the stored edge list — every stored edge counts once, parallel edges and
  self-loops included; ``dist`` -1 = unreachable; ``pred`` = the LARGEST node index among the tight predecessors, -9999 on the source
  and for unreachable nodes;
* the reference's Brandes accumulation: a source contributes ``npred[w] * dep[w]`` to node ``w`` (``npred`` = stored edges into ``w``
  from the previous level, ``dep[v]`` = sum over v's edges to the next level of ``sigma[v] / sigma[w] * (1 + dep[w])``), and the result
  has a key for exactly the nodes some source reached at distance >= 1;
* closeness from per-node totals: ``(r / tot) * (r / (n - 1))`` over INCOMING distances, 0.0 if nothing reaches the node.
"""
from __future__ import annotations

import numpy as np

NO_PRED = -9999


def csr(edge_index, n: int):
    """Source-major CSR of a [2, m] edge list (stable in the edge order)."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    order = np.argsort(ei[0], kind="stable")
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei[0], minlength=n), out=row_ptr[1:])
    return row_ptr, ei[1][order]


def bfs(row_ptr, col, n: int, s: int):
    """(dist [n] int, pred [n] int, levels: list of node lists) of one source."""
    dist = [-1] * n
    pred = [NO_PRED] * n
    dist[s] = 0
    levels = [[s]]
    while levels[-1]:
        d = len(levels) - 1
        nxt = []
        for v in levels[-1]:
            for w in col[row_ptr[v]:row_ptr[v + 1]].tolist():
                if dist[w] < 0:
                    dist[w] = d + 1
                    nxt.append(w)
                if dist[w] == d + 1:
                    pred[w] = max(pred[w], v)
        levels.append(nxt)
    levels.pop()
    return dist, pred, levels


def shortest_paths(edge_index, n: int, sources=None):
    """(dist float64 [k, n] with inf, pred int32 [k, n]) as shortest_paths_dijkstra returns them."""
    row_ptr, col = csr(edge_index, n)
    sources = range(n) if sources is None else sources
    dist = np.full((len(sources), n), np.inf)
    pred = np.full((len(sources), n), NO_PRED, dtype=np.int32)
    for i, s in enumerate(sources):
        d, p, _ = bfs(row_ptr, col, n, s)
        d = np.asarray(d)
        dist[i, d >= 0] = d[d >= 0]
        pred[i] = p
    return dist, pred


def totals(dist):
    """From an all-sources distance matrix: (reach_in [n], dist_in [n], sum of finite off-diagonal distances, largest one,
    number of ordered pairs without a path)."""
    n = dist.shape[0]
    off = ~np.eye(n, dtype=bool)
    finite = np.isfinite(dist) & off
    d = np.where(finite, dist, 0.0).astype(np.int64)
    return finite.sum(axis=0), d.sum(axis=0), int(d.sum()), int(d.max()) if n else 0, int((off & ~finite).sum())


def diameter(dist) -> float:
    if dist.shape[0] <= 1:
        return 0.0
    _, _, _, longest, no_path = totals(dist)
    return float("inf") if no_path else float(longest)


def avg_path_length(dist) -> float:
    n = dist.shape[0]
    if n <= 1:
        return float("nan")
    _, _, total, _, no_path = totals(dist)
    return float("inf") if no_path else float(np.float64(total) / (n * (n - 1)))


def closeness(dist) -> np.ndarray:
    n = dist.shape[0]
    reach_in, dist_in, _, _, _ = totals(dist)
    out = np.zeros(n)
    for v in range(n):
        r, tot = int(reach_in[v]), int(dist_in[v])
        if tot != 0 and n > 1:
            out[v] = (float(r) / float(tot)) * (float(r) / float(n - 1))
    return out


def _expand(row_ptr, col, fr_s, fr_v):
    """Every stored out-edge of the frontier pairs (source row, node): (row, node, neighbour), in frontier order, CSR order inside a node."""
    cnt = row_ptr[fr_v + 1] - row_ptr[fr_v]
    first = np.cumsum(cnt) - cnt
    pos = np.arange(int(cnt.sum())) - np.repeat(first, cnt) + np.repeat(row_ptr[fr_v], cnt)
    return np.repeat(fr_s, cnt), np.repeat(fr_v, cnt), col[pos]


def all_sources(edge_index, n: int, sources=None, brandes: bool = True):
    """The same contract for all sources at once, level by level over (source, node) pairs with numpy — what the tests use where the
    per-source Python loops above would take minutes; the host tests hold it to those loops.  Path counts are float64 here (exact
    below 2**53).  Returns ``dict(dist, pred[, bw, keys])``; ``bw`` sums the sources' contributions in source order."""
    row_ptr, col = csr(edge_index, n)
    sources = np.arange(n) if sources is None else np.asarray(sources, dtype=np.int64)
    k = len(sources)
    rows = np.arange(k)
    D = np.full((k, n), -1, dtype=np.int32)
    D[rows, sources] = 0
    pred = np.full((k, n), NO_PRED, dtype=np.int32)
    sigma = np.zeros((k, n))
    sigma[rows, sources] = 1.0
    npred = np.zeros((k, n), dtype=np.int64)
    fr_s, fr_v, d = rows, sources, 0
    while fr_s.size:
        e_s, e_v, e_w = _expand(row_ptr, col, fr_s, fr_v)
        fresh = D[e_s, e_w] < 0
        D[e_s[fresh], e_w[fresh]] = d + 1
        tight = D[e_s, e_w] == d + 1
        ts, tv, tw = e_s[tight], e_v[tight], e_w[tight]
        np.maximum.at(pred, (ts, tw), tv.astype(np.int32))           # the largest tight predecessor index
        if brandes:
            flat = ts * n + tw
            sigma += np.bincount(flat, weights=sigma[ts, tv], minlength=k * n).reshape(k, n)
            npred += np.bincount(flat, minlength=k * n).reshape(k, n)
        fr_s, fr_v = np.nonzero(D == d + 1)
        d += 1
    dist = np.where(D >= 0, D, np.inf).astype(np.float64)
    out = {"dist": dist, "pred": pred}
    if brandes:
        dep = np.zeros((k, n))
        for level in range(d - 1, 0, -1):
            fr_s, fr_v = np.nonzero(D == level)
            e_s, e_v, e_w = _expand(row_ptr, col, fr_s, fr_v)
            tight = D[e_s, e_w] == level + 1
            ts, tv, tw = e_s[tight], e_v[tight], e_w[tight]
            term = sigma[ts, tv] / sigma[ts, tw] * (1.0 + dep[ts, tw])
            dep += np.bincount(ts * n + tv, weights=term, minlength=k * n).reshape(k, n)       # bincount adds in input (= CSR) order
        bw = np.zeros(n)
        for i in range(k):
            bw += npred[i] * dep[i]
        out["bw"], out["keys"] = bw, (D >= 1).any(axis=0)
    return out


def betweenness(edge_index, n: int, sources=None):
    """(values float64 [n], keys bool [n]) of the reference's betweenness_centrality for the given source INDICES (default: all)."""
    row_ptr, col = csr(edge_index, n)
    values = np.zeros(n)
    keys = np.zeros(n, dtype=bool)
    for s in (range(n) if sources is None else sources):
        dist, _, levels = bfs(row_ptr, col, n, s)
        sigma = [0] * n                       # Python ints: exact
        npred = [0] * n
        sigma[s] = 1
        for level in levels:
            for v in level:
                for w in col[row_ptr[v]:row_ptr[v + 1]].tolist():
                    if dist[w] == dist[v] + 1:
                        sigma[w] += sigma[v]
                        npred[w] += 1
        dep = [0.0] * n
        for level in reversed(levels[1:]):
            for v in level:
                acc = 0.0
                for w in col[row_ptr[v]:row_ptr[v + 1]].tolist():
                    if dist[w] == dist[v] + 1:
                        acc += sigma[v] / sigma[w] * (1 + dep[w])
                dep[v] = acc
                values[v] += npred[v] * acc
                keys[v] = True
    return values, keys
