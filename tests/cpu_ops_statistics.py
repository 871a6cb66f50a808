"""Plain Python / numpy restatement of pathpyG's graph statistics for the tests of pathpyg_amd.statistics: closed triads and clustering
coefficients from Python sets, degree statistics from exact integers and float64, node similarities from sets and dense rows.  It shares
no code with the package and none of its ideas: nothing here sorts a list, bisects, scans or coalesces.

Every function takes the STORED edge list ``edge_index`` [2, m] (row-sorted, parallel edges and self-loops kept) and ``n``; ``undirected``
is the flag of the graph, which changes normalisations only.  Float32 quantities of the reference (moments, generating function) are
returned in float64 from exact inputs: the tests hold them to the float32 rounding bound of the expression, see ``float32_sum_bound``.
"""
import math
from collections import deque
from fractions import Fraction

import numpy as np


def stored_rows(edge_index, n):
    """Successor LISTS in stored order, parallel edges repeated."""
    rows = [[] for _ in range(n)]
    for u, w in np.asarray(edge_index, dtype=np.int64).reshape(2, -1).T.tolist():
        rows[u].append(w)
    return rows


def successor_sets(edge_index, n):
    return [set(r) for r in stored_rows(edge_index, n)]


def in_degrees(edge_index, n):
    return np.bincount(np.asarray(edge_index)[1], minlength=n).astype(np.int64)


def out_degrees(edge_index, n):
    return np.bincount(np.asarray(edge_index)[0], minlength=n).astype(np.int64)


# ------------------------------------------------------------------ clustering
def closed_triads_of(edge_index, n, v, sets=None):
    s = successor_sets(edge_index, n) if sets is None else sets
    return {(x, y) for x in s[v] for y in s[x] if y in s[v]}


def triad_counts(edge_index, n):
    s = successor_sets(edge_index, n)
    return np.array([len(closed_triads_of(edge_index, n, v, s)) for v in range(n)], dtype=np.int64)


def local_coefficients(edge_index, n, undirected):
    deg = in_degrees(edge_index, n) if undirected else out_degrees(edge_index, n)
    out = np.zeros(n, dtype=np.float64)
    for v, (t, d) in enumerate(zip(triad_counts(edge_index, n).tolist(), deg.tolist())):
        if d > 1:
            out[v] = float(Fraction(t, d * (d - 1)))                    # the correctly rounded quotient
    return out


def avg_coefficient(edge_index, n, undirected):
    """The exact mean of the float32 roundings, as a float (``nan`` without nodes)."""
    if n == 0:
        return float("nan")
    rounded = local_coefficients(edge_index, n, undirected).astype(np.float32)
    return float(sum(Fraction(float(c)) for c in rounded) / n)


# ------------------------------------------------------------------ degrees
def degree_sequence(edge_index, n, undirected, mode):
    if mode == "in" or (mode == "total" and undirected):
        return in_degrees(edge_index, n)
    if mode == "out":
        return out_degrees(edge_index, n)
    return in_degrees(edge_index, n) + out_degrees(edge_index, n)


def degree_distribution(edge_index, n, undirected, mode):
    seq = degree_sequence(edge_index, n, undirected, mode)
    return (np.bincount(seq).astype(np.float32) / np.float32(n)).astype(np.float32)


def raw_moment(edge_index, n, undirected, mode, k):
    """``(value, sum of |terms|)`` in float64 from the float32 distribution."""
    p = degree_distribution(edge_index, n, undirected, mode).astype(np.float64)
    terms = np.arange(len(p), dtype=np.float64) ** k * p
    return float(terms.sum()), float(np.abs(terms).sum())


def mean_degree(edge_index, n, undirected, mode):
    return float(np.float32(int(degree_sequence(edge_index, n, undirected, mode).sum())) / np.float32(n))


def central_moment(edge_index, n, undirected, mode, k):
    p = degree_distribution(edge_index, n, undirected, mode).astype(np.float64)
    terms = (np.arange(len(p), dtype=np.float64) - mean_degree(edge_index, n, undirected, mode)) ** k * p
    return float(terms.sum()), float(np.abs(terms).sum())


def stored_m(edge_index, undirected):
    ei = np.asarray(edge_index)
    if not undirected:
        return ei.shape[1]
    loops = int((ei[0] == ei[1]).sum())
    return int((ei.shape[1] - loops) / 2 + loops)


def mean_neighbor_degree(edge_index, n, undirected, mode, exclude_backlink):
    seq = degree_sequence(edge_index, n, undirected, mode) - (1 if exclude_backlink else 0)
    total = int((in_degrees(edge_index, n) * seq).sum())
    m = stored_m(edge_index, undirected)
    return total / (2 * m if undirected else m)                         # ZeroDivisionError without edges, as in the reference


def degree_assortativity(edge_index, n, undirected, mode):
    seq = [int(d) for d in degree_sequence(edge_index, n, undirected, mode)]
    ei = np.asarray(edge_index)
    s1, s2, s3 = (float(sum(d ** p for d in seq)) for p in (1, 2, 3))
    se = float(sum(seq[u] * seq[w] for u, w in ei.T.tolist()))
    return (s1 * se - s2 ** 2) / (s1 * s3 - s2 ** 2)


def generating_function(edge_index, n, undirected, mode, x):
    """``(values, sums of |terms|)`` in float64 at the float32 roundings of ``x``."""
    p = degree_distribution(edge_index, n, undirected, mode).astype(np.float64)
    x = np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1)
    terms = p[:, None] * x[None, :] ** np.arange(len(p))[:, None]
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def float32_sum_bound(count, magnitude):
    """Bound on |float32 evaluation - exact value| of a sum of ``count`` float32 products whose absolute values add up to ``magnitude``:
    every term carries at most three roundings (power, product, the operand itself) and the sum at most ``count`` more, each relative
    2**-24; one float32 ulp of slack for the value the reference read back."""
    return (count + 4) * 2.0 ** -24 * magnitude * 1.0001 + 2.0 ** -126


# ------------------------------------------------------------------ node similarities
def common_neighbors(edge_index, n, v, w, sets=None):
    s = successor_sets(edge_index, n) if sets is None else sets
    return len(s[v] & s[w])


def overlap(edge_index, n, v, w):
    s = successor_sets(edge_index, n)
    return len(s[v] & s[w]) / min(len(s[v]), len(s[w]))                 # ZeroDivisionError when a set is empty


def jaccard(edge_index, n, v, w):
    s = successor_sets(edge_index, n)
    if not s[v] and not s[w]:
        return 1
    return len(s[v] & s[w]) / len(s[v] | s[w])


def adamic_adar_terms(edge_index, n, v, w):
    """The terms ``1 / log(out-degree)`` of the common successors, ascending by node (``inf`` at degree 1, ``-0.0`` at degree 0)."""
    s, deg = successor_sets(edge_index, n), out_degrees(edge_index, n)
    with np.errstate(divide="ignore"):
        return [float(1 / np.log(int(deg[u]))) for u in sorted(s[v] & s[w])]


def adamic_adar(edge_index, n, v, w):
    return math.fsum(t for t in adamic_adar_terms(edge_index, n, v, w)) if adamic_adar_terms(edge_index, n, v, w) else 0


def cosine(edge_index, n, v, w):
    ind = in_degrees(edge_index, n)
    if ind[v] == 0 or ind[w] == 0:
        return 0
    dense = np.zeros((n, n))
    for a, b in np.asarray(edge_index).T.tolist():
        dense[a, b] += 1
    with np.errstate(invalid="ignore"):
        return np.dot(dense[v], dense[w]) / (math.sqrt(np.dot(dense[v], dense[v])) * math.sqrt(np.dot(dense[w], dense[w]))) \
            if dense[v].any() and dense[w].any() else float("nan")


def inverse_path_length(edge_index, n, v, w, undirected):
    if v == w:
        return float("inf")
    rows = stored_rows(edge_index, n)
    if undirected:
        for a, b in np.asarray(edge_index).T.tolist():
            rows[b].append(a)
    dist, queue = {v: 0}, deque([v])
    while queue:
        a = queue.popleft()
        for b in rows[a]:
            if b not in dist:
                dist[b] = dist[a] + 1
                queue.append(b)
    return 1 / dist[w] if w in dist else 0.0


def pair_table(edge_index, n, pairs):
    """Every pair measure for many index pairs from ONE pass over the edge list: a dict of lists in the order of ``pairs`` ([2, P]) with
    ``common`` (ints), ``overlap`` and ``jaccard`` and ``cosine`` (floats, ``nan`` where the scalar function raises or the reference gives
    nan), ``terms`` (the Adamic-Adar terms of each pair, ascending by node) and ``sizes``."""
    from collections import Counter
    rows = [Counter(r) for r in stored_rows(edge_index, n)]
    sets = [set(r) for r in rows]
    ind, deg = in_degrees(edge_index, n), out_degrees(edge_index, n)
    norm = [sum(c * c for c in r.values()) for r in rows]
    out = {"common": [], "overlap": [], "jaccard": [], "cosine": [], "terms": [], "sizes": []}
    with np.errstate(divide="ignore"):
        for v, w in np.asarray(pairs, dtype=np.int64).reshape(2, -1).T.tolist():
            both = sets[v] & sets[w]
            least = min(len(sets[v]), len(sets[w]))
            out["common"].append(len(both))
            out["sizes"].append((len(sets[v]), len(sets[w])))
            out["overlap"].append(len(both) / least if least else float("nan"))
            out["jaccard"].append(1.0 if not sets[v] and not sets[w] else len(both) / len(sets[v] | sets[w]))
            if ind[v] == 0 or ind[w] == 0:
                out["cosine"].append(0.0)
            elif not norm[v] or not norm[w]:
                out["cosine"].append(float("nan"))
            else:
                out["cosine"].append(sum(rows[v][u] * rows[w][u] for u in both) / (math.sqrt(norm[v]) * math.sqrt(norm[w])))
            out["terms"].append([float(1 / np.log(int(deg[u]))) for u in sorted(both)])
    return out
