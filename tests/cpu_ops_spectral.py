"""Plain numpy restatement of networkx 3.4's ``eigenvector_centrality`` and ``katz_centrality`` loops over an edge list, as the reference
reaches them: on a DiGraph of the DISTINCT edges (parallel edges collapse, self-loops stay, isolated nodes are present), unit weights unless
weights are given, in which case an entry's weight is the sum over its parallel edges.  Only the summation ORDER differs from networkx
(``np.bincount`` adds a node's terms in edge order, ``np.sum`` is pairwise), so values agree to rounding and — for inputs whose error never
comes within rounding of the threshold — the iteration counts are equal."""
from __future__ import annotations

import math

import numpy as np


class FailedConvergence(Exception):
    def __init__(self, max_iter):
        super().__init__(f"no convergence within {max_iter} iterations")
        self.max_iter = max_iter


def simple_edges(edge_index, n: int, weights=None):
    """``(src, dst, w)`` of the distinct edges, (src, dst)-sorted; ``w`` = the summed weights, or ones."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    if ei.shape[1] == 0:
        return ei[0], ei[1], np.zeros(0)
    keys, inverse = np.unique(ei[0] * n + ei[1], return_inverse=True)
    w = np.ones(keys.size) if weights is None else np.bincount(inverse.reshape(-1), weights=np.asarray(weights, dtype=np.float64), minlength=keys.size)
    return keys // n, keys % n, w


def _vector(value, n: int, default: float):
    if value is None:
        return np.full(n, default, dtype=np.float64)
    if isinstance(value, dict):
        return np.array([float(value[i]) for i in range(n)])
    return np.asarray(value, dtype=np.float64).reshape(n).copy()


def eigenvector(edge_index, n: int, max_iter: int = 100, tol: float = 1e-06, nstart=None, weights=None):
    """``(values [n], iterations)``; ``ValueError`` for the null graph and an all-zero start, :class:`FailedConvergence` otherwise."""
    if n == 0:
        raise ValueError("cannot compute centrality for the null graph")
    src, dst, w = simple_edges(edge_index, n, weights)
    x = _vector(nstart, n, 1.0)
    if not x.any():
        raise ValueError("initial vector cannot have all zero values")
    with np.errstate(all="ignore"):
        x = x / x.sum()
        for it in range(1, max_iter + 1):
            y = x + np.bincount(dst, weights=w * x[src], minlength=n)
            norm = np.sqrt(np.sum(y * y)) or 1.0
            new = y / norm
            if np.sum(np.abs(new - x)) < n * tol:
                return new, it
            x = new
    raise FailedConvergence(max_iter)


def katz(edge_index, n: int, alpha: float = 0.1, beta=1.0, max_iter: int = 1000, tol: float = 1e-06, nstart=None, normalized: bool = True,
         weights=None):
    """``(values [n], iterations)``; an empty result for the null graph."""
    if n == 0:
        return np.zeros(0), 0
    src, dst, w = simple_edges(edge_index, n, weights)
    x = _vector(nstart, n, 0.0)
    b = np.full(n, float(beta)) if np.isscalar(beta) else _vector(beta, n, 0.0)
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            new = alpha * np.bincount(dst, weights=w * x[src], minlength=n) + b
            if np.sum(np.abs(new - x)) < n * tol:
                norm = np.sqrt(np.sum(new * new)) if normalized else 1.0
                return new * (1.0 / norm if norm != 0.0 else 1.0), it
            x = new
    raise FailedConvergence(max_iter)


def katz_exact(edge_index, n: int, iterations: int, alpha: float = 0.1, beta=1.0, nstart=None, normalized: bool = True, weights=None):
    """Exactly ``iterations`` Katz iterations with exactly rounded sums (``math.fsum`` per row and for the norm), no test: what the
    fixture generator measures networkx against."""
    src, dst, w = (a.tolist() for a in simple_edges(edge_index, n, weights))
    rows = [[] for _ in range(n)]
    for u, v, t in zip(src, dst, w):
        rows[v].append((u, t))
    x = _vector(nstart, n, 0.0).tolist()
    b = [float(beta)] * n if np.isscalar(beta) else _vector(beta, n, 0.0).tolist()
    for _ in range(iterations):
        x = [alpha * math.fsum(x[u] * t for u, t in rows[v]) + b[v] for v in range(n)]
    norm = math.sqrt(math.fsum(t * t for t in x)) if normalized else 1.0
    return np.array(x) * (1.0 / norm if norm != 0.0 else 1.0)


def derived_rtol(values, exact) -> float:
    """The fixtures' bound for a case made here: 16 x the rtol needed between ``values`` (sums in some order) and ``exact`` (the same
    iterations, exactly rounded sums), floor 2**-48; form of tests/tolerance.py with ``values`` as the reference."""
    rms = float(np.sqrt(np.mean(values * values))) if values.size else 0.0
    needed = float(np.max(np.abs(exact - values) / (np.abs(values) + rms + 1e-300))) if values.size else 0.0
    return max(2.0 ** -48, 16.0 * needed)
