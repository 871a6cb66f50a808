#!/usr/bin/env python3
"""Generate tests/golden/pagerank_vectors.npz from ``networkx.pagerank``.

Needs networkx (3.4, with scipy) and numpy only.  The graphs are those of make_golden_spectral.graphs(); the copy networkx sees is its
``digraph``: a ``DiGraph`` with nodes ``0 .. n-1`` and the DISTINCT stored edges, self-loops kept, and for the weighted cases (an extension
of this project) the ``weight`` of an edge summed over its parallel edges.

    python tests/golden/make_golden_pagerank.py

The file holds ``graphs`` (names) with ``graph/<g>/edge_index`` int32 [2, m] and ``graph/<g>/n``, and ``names`` (cases) with, per case
``<c>``: ``/graph``, the arguments ``/alpha``, ``/max_iter``, ``/tol``, ``/personalization``, ``/nstart``, ``/dangling`` ([0] = none, else [n]),
``/personalization_keys`` and ``/personalization_values`` (a PARTIAL dict; [0] = none), ``/weights`` ([0] = none, else one value per stored
edge); the results ``/raised``, ``/values`` (networkx's, float64 [n]; [0] if it raised), ``/iterations`` (networkx's loop is restated below
to count, and the restatement is checked against networkx bit for bit), ``/margin`` = the smallest ``|err / (n tol) - 1|`` over all
iterations and ``/rtol``: 16 times the rtol needed between networkx's values and the same number of iterations run with exactly rounded sums
(``math.fsum`` per row and for the dangling mass) on the CONTRACT's probabilities ``w / T_u`` (networkx multiplies by a rounded ``1 / T_u``),
floor 2**-48, in the form of tests/tolerance.py.

Every case is asserted to have margin >= 1e-6: rounding moves ``err`` by about 1e-13 relative, so no correct implementation can stop an
iteration earlier or later than networkx.
"""
from __future__ import annotations

import math
import pathlib
import sys

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
from make_golden_spectral import FLOOR, digraph, graphs, rtol_needed  # noqa: E402


def vector(given, n):
    """networkx's normalisation of a dict argument: ``[d.get(v, 0) for v in nodelist] / sum``."""
    if given is None:
        return np.repeat(1.0 / n, n)
    v = np.array([given.get(i, 0) for i in range(n)], dtype=float)
    return v / v.sum()


def restated(nx, g, *, alpha, max_iter, tol, personalization, nstart, dangling, weighted):
    """networkx 3.4's ``_pagerank_scipy`` loop: ``(values | None, iterations, margin)``."""
    import scipy as sp

    n = len(g)
    nodelist = list(g)
    A = nx.to_scipy_sparse_array(g, nodelist=nodelist, weight="weight" if weighted else None, dtype=float)
    S = A.sum(axis=1)
    S[S != 0] = 1.0 / S[S != 0]
    Q = sp.sparse.csr_array(sp.sparse.spdiags(S.T, 0, *A.shape))
    A = Q @ A
    x = vector(nstart, n)
    p = vector(personalization, n)
    dangling_weights = p if dangling is None else vector(dangling, n)
    is_dangling = np.where(S == 0)[0]
    margin = math.inf
    for it in range(1, max_iter + 1):
        xlast = x
        x = alpha * (x @ A + sum(x[is_dangling]) * dangling_weights) + (1 - alpha) * p
        err = np.absolute(x - xlast).sum()
        margin = min(margin, abs(err / (n * tol) - 1))
        if err < n * tol:
            return x, it, margin
    return None, max_iter, margin


def exact(g, iterations, *, alpha, personalization, nstart, dangling, weighted):
    """``iterations`` iterations with exactly rounded sums on the contract's probabilities ``w / T_u``, ``T_u`` the left-to-right sum of u's
    out-entries in ascending target order."""
    n = len(g)
    w = {u: sorted((v, float(d.get("weight", 1)) if weighted else 1.0) for v, d in g[u].items()) for u in g}
    T = {}
    for u in g:
        s = 0.0
        for _, x in w[u]:
            s = s + x
        T[u] = s
    pred = {v: [] for v in g}
    for u in g:
        for v, x in w[u]:
            pred[v].append((u, x / T[u] if T[u] > 0 else 0.0))
    dang = [u for u in g if not T[u] > 0]
    x = vector(nstart, n).tolist()
    p = vector(personalization, n).tolist()
    d = p if dangling is None else vector(dangling, n).tolist()
    for _ in range(iterations):
        D = math.fsum(x[u] for u in dang)
        x = [alpha * (math.fsum(pr * x[u] for u, pr in pred[v]) + D * d[v]) + (1 - alpha) * p[v] for v in range(n)]
    return np.array(x)


def cases(gs):
    """(case name, graph, arguments)"""
    rng = np.random.default_rng(2025)
    for g in gs:
        yield f"{g}_pr", g, {}
    n300, m300 = gs["random_300"][1], gs["random_300"][0].shape[1]
    first_multi = next(k for k in gs if k.startswith("multi_"))
    nm, mm = gs[first_multi][1], gs[first_multi][0].shape[1]
    yield "random_300_weighted", "random_300", dict(weights=rng.uniform(0.5, 1.5, m300))
    yield "random_50_weighted", "random_50", dict(weights=rng.uniform(0.5, 1.5, gs["random_50"][0].shape[1]))
    yield f"{first_multi}_weighted", first_multi, dict(weights=rng.uniform(0.5, 1.5, mm))
    yield "in_hub_weighted", "in_hub", dict(weights=rng.uniform(0.5, 1.5, gs["in_hub"][0].shape[1]))
    yield "random_300_alpha_half", "random_300", dict(alpha=0.5)
    yield "random_300_alpha_one", "random_300", dict(alpha=1.0, max_iter=500)
    yield "k5_alpha_one", "k5", dict(alpha=1.0)
    yield "hub_ring_alpha_half", "hub_ring", dict(alpha=0.5)
    yield "random_300_personalization", "random_300", dict(personalization=dict(enumerate(rng.uniform(0.0, 1.0, n300).tolist())))
    yield "random_300_partial", "random_300", dict(personalization={3: 1.0, 17: 2.0, 250: 0.5})
    yield "in_hub_partial", "in_hub", dict(personalization={0: 1.0, 4999: 3.0})
    yield "random_300_nstart", "random_300", dict(nstart=dict(enumerate(rng.uniform(0.1, 1.0, n300).tolist())))
    yield f"{first_multi}_dangling", first_multi, dict(dangling=dict(enumerate(rng.uniform(0.0, 1.0, nm).tolist())))
    yield "path3_dangling", "path3", dict(dangling={0: 1.0, 1: 3.0})
    yield "random_300_tol", "random_300", dict(tol=1e-12, max_iter=500)
    yield "random_3000_raises", "random_3000", dict(max_iter=3)
    yield f"{first_multi}_all", first_multi, dict(alpha=0.7, weights=rng.uniform(0.5, 1.5, mm), personalization={0: 1.0, 1: 1.0},
                                                  nstart=dict(enumerate(rng.uniform(0.1, 1.0, nm).tolist())), dangling={2: 1.0}, tol=1e-9)


def dense(given, n):
    return np.zeros(0) if given is None else np.array([given.get(i, 0) for i in range(n)], dtype=np.float64)


def main() -> int:
    import networkx as nx

    gs = graphs()
    store = {"graphs": np.array(list(gs))}
    for g, (ei, n) in gs.items():
        store[f"graph/{g}/edge_index"] = ei.astype(np.int32)
        store[f"graph/{g}/n"] = np.int64(n)
    names, worst_margin, worst_rtol = [], math.inf, 0.0
    for name, g, given in cases(gs):
        ei, n = gs[g]
        args = dict(alpha=0.85, max_iter=100, tol=1e-06, personalization=None, nstart=None, dangling=None, weights=None)
        args.update(given)
        weights = args.pop("weights")
        weighted = weights is not None
        nxg = digraph(nx, ei, n, weights)
        mine, iterations, margin = restated(nx, nxg, weighted=weighted, **args)
        try:
            got = nx.pagerank(nxg, weight="weight" if weighted else None, **args)
        except nx.PowerIterationFailedConvergence:
            got = None
        assert (got is None) == (mine is None), name
        assert margin >= 1e-6, (name, margin)
        rtol, values = FLOOR, np.zeros(0)
        if got is not None:
            values = np.array([got[v] for v in range(n)], dtype=np.float64)
            assert np.array_equal(values, mine), name                                   # the restatement IS networkx's loop
            yard = exact(nxg, iterations, weighted=weighted, **{k: args[k] for k in ("alpha", "personalization", "nstart", "dangling")})
            rtol = max(FLOOR, 16 * rtol_needed(values, yard))
            worst_rtol = max(worst_rtol, rtol)
        worst_margin = min(worst_margin, margin)
        partial = args["personalization"] is not None and len(args["personalization"]) < n
        store[f"{name}/graph"] = np.array(g)
        store[f"{name}/alpha"] = np.float64(args["alpha"])
        store[f"{name}/max_iter"] = np.int64(args["max_iter"])
        store[f"{name}/tol"] = np.float64(args["tol"])
        store[f"{name}/personalization"] = np.zeros(0) if partial else dense(args["personalization"], n)
        store[f"{name}/personalization_keys"] = np.array(sorted(args["personalization"]), dtype=np.int64) if partial else np.zeros(0, dtype=np.int64)
        store[f"{name}/personalization_values"] = (np.array([args["personalization"][k] for k in sorted(args["personalization"])], dtype=np.float64)
                                                   if partial else np.zeros(0))
        store[f"{name}/nstart"] = dense(args["nstart"], n)
        store[f"{name}/dangling"] = dense(args["dangling"], n)
        store[f"{name}/weights"] = np.zeros(0) if weights is None else weights
        store[f"{name}/raised"] = np.bool_(got is None)
        store[f"{name}/values"] = values
        store[f"{name}/iterations"] = np.int64(iterations)
        store[f"{name}/margin"] = np.float64(margin)
        store[f"{name}/rtol"] = np.float64(rtol)
        names.append(name)
        print(f"{name:34s} n {n:5d} {'raised' if got is None else 'stops '} at {iterations:5d}  margin {margin:.2e}  rtol {rtol:.2e}")
    store["names"] = np.array(names)
    path = OUT / "pagerank_vectors.npz"
    np.savez_compressed(path, **store)
    print(f"{len(names)} cases -> {path} ({path.stat().st_size} bytes); smallest margin {worst_margin:.2e}, largest rtol {worst_rtol:.2e}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
