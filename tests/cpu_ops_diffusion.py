"""Host restatements of the propagator of csrc/pp_graph_diffusion.hip (the header's "distributions and PageRank" block), in two grades:

* the YARDSTICK: the contract's iteration with exactly rounded sums (``math.fsum`` per row, for the dangling mass, the error and tvd) on the
  contract's probabilities ``w / T_u`` — what every summation order is within rounding of;
* the NUMPY restatement: the same iteration as dense float64 matrix products, whose distance to the yardstick is the size of the rounding
  the tests allow a multiple of.

``merged`` is the structure the kernels see: the distinct edges sorted by (source, target), an entry weighing 1, its stored edges
(``count_stored``: RandomWalk's view of ``weight=None``) or the sum of a weight over them.
"""
from __future__ import annotations

import math

import numpy as np


def merged(edge_index, n: int, weights=None, count_stored: bool = False):
    """``(src, dst, w)`` of the merged entries, sorted by (src, dst); parallel edges' weights are added in stored order."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    order = np.argsort(ei[0], kind="stable")                    # the Graph constructor's stable sort by source
    total: dict = {}
    for j in order.tolist():
        key = (int(ei[0, j]), int(ei[1, j]))
        w = 1.0 if weights is None else float(weights[j])
        if key in total:
            total[key] = total[key] + w if (weights is not None or count_stored) else 1.0
        else:
            total[key] = w
    keys = sorted(total)
    src = np.array([k[0] for k in keys], dtype=np.int64)
    dst = np.array([k[1] for k in keys], dtype=np.int64)
    return src, dst, np.array([total[k] for k in keys], dtype=np.float64)


def table(src, dst, w, n: int):
    """``(T [n], prob [k], dangling [n] bool)``: T_u the left-to-right sum of u's entries, prob = w / T_u (0 where T_u is 0)."""
    T = np.zeros(n)
    for u, x in zip(src.tolist(), w.tolist()):
        T[u] = T[u] + x
    prob = np.array([x / T[u] if T[u] > 0 else 0.0 for u, x in zip(src.tolist(), w.tolist())], dtype=np.float64)
    return T, prob, ~(T > 0)


def dense_matrix(src, dst, prob, dangling, n: int, lazy: float = 0.0, keep_dangling: bool = True) -> np.ndarray:
    """``M`` with ``x' = x @ M`` for the walk mode: ``lazy I + (1 - lazy) (P + diag(dangling))``; ``keep_dangling=False``: P alone."""
    P = np.zeros((n, n))
    P[src, dst] = prob
    if not keep_dangling:
        return P
    P[np.arange(n)[dangling], np.arange(n)[dangling]] += 1.0
    return lazy * np.eye(n) + (1.0 - lazy) * P


def pull_lists(src, dst, prob, n: int) -> list:
    lists = [[] for _ in range(n)]
    for u, v, p in zip(src.tolist(), dst.tolist(), prob.tolist()):
        lists[v].append((u, p))
    return lists


def walk_step_exact(x, lists, dangling, lazy: float) -> list:
    """One walk-mode iteration with exactly rounded row sums: the contract's operations, ``math.fsum`` for the sum."""
    return [lazy * x[v] + (1.0 - lazy) * (math.fsum(p * x[u] for u, p in lists[v]) + (x[v] if dangling[v] else 0.0)) for v in range(len(x))]


def evolve_exact(x0, src, dst, prob, dangling, n: int, steps: int, lazy: float = 0.0) -> np.ndarray:
    """``[steps + 1, n]``: the yardstick trajectory of one start distribution."""
    lists = pull_lists(src, dst, prob, n)
    out = [list(map(float, x0))]
    for _ in range(steps):
        out.append(walk_step_exact(out[-1], lists, dangling.tolist(), lazy))
    return np.array(out)


def evolve_numpy(x0, M: np.ndarray, steps: int) -> np.ndarray:
    """``[steps + 1, n]`` (or ``[steps + 1, n, B]`` for a block): the dense restatement, ``x @ M`` per step."""
    out = [np.asarray(x0, dtype=np.float64)]
    for _ in range(steps):
        out.append((out[-1].T @ M).T)
    return np.array(out)


def evolve_bincount(x0, src, dst, prob, dangling, n: int, steps: int, lazy: float = 0.0) -> np.ndarray:
    """``[steps + 1, n]``: the float64 restatement for graphs too large for a dense matrix — ``numpy.bincount`` adds a row's terms one after
    the other in entry order."""
    out = [np.asarray(x0, dtype=np.float64)]
    for _ in range(steps):
        x = out[-1]
        s = np.bincount(dst, weights=prob * x[src], minlength=n)
        out.append(lazy * x + (1.0 - lazy) * (s + np.where(dangling, x, 0.0)))
    return np.array(out)


def stationary_numpy(x0, M: np.ndarray, tol: float, max_iter: int):
    """``(x | None, iterations)`` of the dense restatement with the contract's stopping rule: the first iterate with sum |x' - x| < tol."""
    x = np.asarray(x0, dtype=np.float64)
    for it in range(1, max_iter + 1):
        last, x = x, x @ M
        if np.abs(x - last).sum() < tol:
            return x, it
    return None, max_iter


def pagerank_exact(x0, p, d, src, dst, prob, dangling, n: int, alpha: float, iterations: int) -> np.ndarray:
    """``iterations`` PageRank iterations with exactly rounded sums (the yardstick of tests/golden/make_golden_pagerank.py)."""
    lists = pull_lists(src, dst, prob, n)
    dang = np.flatnonzero(dangling).tolist()
    x = list(map(float, x0))
    for _ in range(iterations):
        D = math.fsum(x[u] for u in dang)
        x = [alpha * (math.fsum(pr * x[u] for u, pr in lists[v]) + D * float(d[v])) + (1.0 - alpha) * float(p[v]) for v in range(n)]
    return np.array(x)


def tvd(x, target) -> np.ndarray:
    """``0.5 * sum |x - target|`` over the node axis (axis 1 of ``[t, n]`` / ``[t, n, B]``)."""
    x, target = np.asarray(x), np.asarray(target)
    shape = (1, -1) + (1,) * (x.ndim - 2)
    return 0.5 * np.abs(x - target.reshape(shape)).sum(axis=1)


def rtol_needed(got, want) -> float:
    """The smallest rtol of tests/tolerance.py's form: ``max |got - want| / (|want| + rms(want))``."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rms = math.sqrt(float(np.mean(want * want))) if want.size else 0.0
    return float(np.max(np.abs(got - want) / (np.abs(want) + rms + 1e-300))) if want.size else 0.0


def dominant_left_eigenvector(M: np.ndarray) -> np.ndarray:
    """The left eigenvector of the eigenvalue nearest 1, scaled to sum 1 (numpy.linalg.eig)."""
    values, vectors = np.linalg.eig(M.T)
    v = np.real(vectors[:, int(np.argmin(np.abs(values - 1.0)))])
    return v / v.sum()
