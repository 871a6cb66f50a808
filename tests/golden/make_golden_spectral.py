#!/usr/bin/env python3
"""Generate tests/golden/spectral_centrality_vectors.npz from networkx's ``eigenvector_centrality`` and ``katz_centrality``.

Needs networkx (3.4) and numpy only, no checkout of the reference.  The reference reaches both functions by forwarding the name to networkx
on ``to_networkx(graph.data)``: a ``DiGraph`` with nodes ``0 .. n-1`` and the stored edges, without attributes.  That copy is rebuilt here
with ``add_nodes_from(range(n))`` and ``add_edges_from(edge_index.T)``; for the weighted cases (an extension of this project) the ``weight``
attribute of an edge is the sum of the given values over its parallel edges.

    python tests/golden/make_golden_spectral.py

The file holds ``graphs`` (names) with ``graph/<g>/edge_index`` int32 [2, m] and ``graph/<g>/n``, and ``names`` (cases) with, per case
``<c>``: ``/graph``, ``/kind`` ("eigenvector" | "katz"), the arguments ``/max_iter``, ``/tol``, ``/alpha``, ``/beta`` ([1] or [n]),
``/nstart`` ([0] = none, else [n]), ``/normalized``, ``/weights`` ([0] = none, else one value per stored edge); the results ``/raised``,
``/values`` (networkx's, float64 [n]; [0] if it raised), ``/iterations`` (where networkx stopped: both loops are restated below to count,
and the restatement is checked against networkx bit for bit), ``/margin`` = the smallest ``|err / (n tol) - 1|`` over all iterations, and
``/rtol``: 16 times the rtol needed between networkx's values and the same number of iterations run with exactly rounded sums
(``math.fsum`` per row and for the norms), floor 2**-48, in the form of tests/tolerance.py: ``|got - want| <= rtol |want| + rtol rms(want)``.
The device's sums carry the same kind of rounding as networkx's, in another order; the factor covers the spread between two such orders.

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
from make_golden_static_paths import cases as static_path_cases  # noqa: E402  (the seeded multigraphs)

FLOOR = 2.0 ** -48


def digraph(nx, edge_index, n, weights=None):
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    if weights is None:
        g.add_edges_from(edge_index.T.tolist())
    else:
        total = {}
        for (u, v), w in zip(edge_index.T.tolist(), weights.tolist()):
            total[(u, v)] = total.get((u, v), 0.0) + w
        g.add_weighted_edges_from((u, v, w) for (u, v), w in total.items())
    return g


def restated(g, kind, weighted, exact_iterations=None, *, max_iter, tol, alpha, beta, nstart, normalized):
    """networkx's loop in networkx's order of operations: ``(values | None, iterations, margin)``.  With ``exact_iterations`` every sum is
    ``math.fsum`` and exactly that many iterations run without a test."""
    n = len(g)
    exact = exact_iterations is not None
    add = math.fsum if exact else sum
    pred = {v: [(u, d.get("weight", 1) if weighted else 1) for u, d in g.pred[v].items()] for v in g}
    margin = math.inf
    if kind == "eigenvector":
        x = {v: 1 for v in g} if nstart is None else dict(enumerate(nstart.tolist()))
        total = add(x.values())
        x = {v: t / total for v, t in x.items()}
    else:
        x = {v: 0 for v in g} if nstart is None else dict(enumerate(nstart.tolist()))
        b = dict.fromkeys(g, float(beta[0])) if beta.size == 1 else dict(enumerate(beta.tolist()))
    for it in range(1, (exact_iterations if exact else max_iter) + 1):
        last = x
        if kind == "eigenvector":
            if exact:
                x = {v: math.fsum([last[v]] + [last[u] * w for u, w in pred[v]]) for v in g}
            else:                                                   # networkx pushes along successors, in node order
                x = last.copy()
                for u in x:
                    for v in g[u]:
                        x[v] += last[u] * (g[u][v].get("weight", 1) if weighted else 1)
            norm = (math.sqrt(math.fsum(t * t for t in x.values())) if exact else math.hypot(*x.values())) or 1
            x = {v: t / norm for v, t in x.items()}
        else:
            if exact:
                x = {v: alpha * math.fsum(last[u] * w for u, w in pred[v]) + b[v] for v in g}
            else:
                x = dict.fromkeys(last, 0)
                for u in x:
                    for v in g[u]:
                        x[v] += last[u] * (g[u][v].get("weight", 1) if weighted else 1)
                for v in x:
                    x[v] = alpha * x[v] + b[v]
        err = add(abs(x[v] - last[v]) for v in x)
        if exact:
            continue
        if not math.isnan(err):
            margin = min(margin, abs(err / (n * tol) - 1))
        if err < n * tol:
            if kind == "katz":
                s = 1.0
                if normalized:
                    try:
                        s = 1.0 / math.hypot(*x.values())
                    except ZeroDivisionError:
                        s = 1.0
                x = {v: t * s for v, t in x.items()}
            return x, it, margin
    if exact:
        if kind == "katz" and normalized:
            norm = math.sqrt(math.fsum(t * t for t in x.values()))
            x = {v: t * (1.0 / norm if norm else 1.0) for v, t in x.items()}
        return x, exact_iterations, margin
    return None, max_iter, margin


def rtol_needed(got, want):
    rms = math.sqrt(float(np.mean(want * want))) if want.size else 0.0
    return float(np.max(np.abs(got - want) / (np.abs(want) + rms + 1e-300))) if want.size else 0.0


def graphs():
    out = {}
    for n, m, seed in ((50, 400, 11), (300, 3000, 12), (3000, 30000, 13)):
        out[f"random_{n}"] = (np.random.default_rng(seed).integers(0, n, (2, m)), n)
    n = 5001
    i = np.arange(1, n)
    zero = np.zeros(n - 1, dtype=np.int64)
    ring = i % (n - 1) + 1
    out["hub_ring"] = (np.concatenate([np.stack([i, zero]), np.stack([zero, i]), np.stack([i, ring])], axis=1), n)
    out["in_hub"] = (np.concatenate([np.stack([i, zero]), np.stack([i, ring]), np.array([[0], [1]])], axis=1), n)
    out["path3"] = (np.array([[0, 1], [1, 2]]), 3)
    out["k5"] = (np.array([(u, v) for u in range(5) for v in range(5) if u != v]).T, 5)
    out["single"] = (np.zeros((2, 0), dtype=np.int64), 1)
    out["single_loop"] = (np.array([[0], [0]]), 1)
    out["isolated3"] = (np.zeros((2, 0), dtype=np.int64), 3)
    multi = [(name, ei, n) for name, ei, n, _ in static_path_cases() if name.startswith("random_") and ei.shape[1] >= 12]
    for name, ei, n in multi[:3]:
        out[f"multi_{name[-2:]}"] = (ei, n)
    return {k: (np.asarray(ei, dtype=np.int64).reshape(2, -1), n) for k, (ei, n) in out.items()}


def cases(gs):
    """(case name, graph, kind, arguments)"""
    E, K = "eigenvector", "katz"
    rng = np.random.default_rng(2024)
    for g in ("random_50", "random_300", "random_3000"):
        yield f"{g}_eig", g, E, {}
        yield f"{g}_katz", g, K, dict(alpha=0.05)
    yield "hub_ring_eig", "hub_ring", E, dict(max_iter=1000)
    yield "hub_ring_katz", "hub_ring", K, dict(alpha=0.01)
    yield "in_hub_eig", "in_hub", E, {}
    yield "in_hub_katz", "in_hub", K, dict(alpha=0.1)
    yield "path3_eig_raises", "path3", E, {}
    yield "path3_katz", "path3", K, {}
    yield "k5_eig", "k5", E, {}
    yield "k5_katz_diverges", "k5", K, dict(alpha=0.5, max_iter=50)
    yield "k5_katz_nan", "k5", K, dict(alpha=0.5, max_iter=1200)
    yield "single_eig", "single", E, {}
    yield "single_katz", "single", K, {}
    yield "single_loop_eig", "single_loop", E, {}
    yield "isolated3_katz", "isolated3", K, {}
    for g in (k for k in gs if k.startswith("multi_")):
        yield f"{g}_eig", g, E, dict(max_iter=500)
        yield f"{g}_katz", g, K, dict(alpha=0.05)
    n = gs["random_300"][1]
    yield "random_300_katz_unnormalized", "random_300", K, dict(alpha=0.05, normalized=False)
    yield "random_300_katz_beta_vector", "random_300", K, dict(alpha=0.05, beta=rng.uniform(0.5, 1.5, n))
    yield "random_300_katz_nstart", "random_300", K, dict(alpha=0.05, nstart=rng.uniform(0.0, 2.0, n))
    yield "random_300_eig_nstart", "random_300", E, dict(nstart=rng.uniform(0.1, 1.0, n))
    yield "random_300_eig_tol", "random_300", E, dict(tol=1e-10, max_iter=300)
    yield "random_300_katz_tol", "random_300", K, dict(alpha=0.05, tol=1e-3)
    yield "random_300_katz_weighted", "random_300", K, dict(alpha=0.05, weights=rng.uniform(0.5, 1.5, gs["random_300"][0].shape[1]))
    first_multi = next(k for k in gs if k.startswith("multi_"))
    yield f"{first_multi}_eig_weighted", first_multi, E, dict(max_iter=500, weights=rng.uniform(0.5, 1.5, gs[first_multi][0].shape[1]))
    yield "random_50_eig_weighted", "random_50", E, dict(weights=rng.uniform(0.5, 1.5, gs["random_50"][0].shape[1]))


def main() -> int:
    import networkx as nx

    gs = graphs()
    store = {"graphs": np.array(list(gs))}
    for g, (ei, n) in gs.items():
        store[f"graph/{g}/edge_index"] = ei.astype(np.int32)
        store[f"graph/{g}/n"] = np.int64(n)
    names, worst_margin, worst_rtol = [], math.inf, 0.0
    for name, g, kind, given in cases(gs):
        ei, n = gs[g]
        eig = kind == "eigenvector"
        args = dict(max_iter=100 if eig else 1000, tol=1e-06, alpha=0.1, beta=1.0, nstart=None, normalized=True, weights=None)
        args.update(given)
        weights = args.pop("weights")
        beta = np.atleast_1d(np.asarray(args["beta"], dtype=np.float64))
        nxg = digraph(nx, ei, n, weights)
        weighted = weights is not None
        loop = dict(max_iter=args["max_iter"], tol=args["tol"], alpha=args["alpha"], beta=beta, nstart=args["nstart"], normalized=args["normalized"])
        mine, iterations, margin = restated(nxg, kind, weighted, **loop)
        nstart = None if args["nstart"] is None else dict(enumerate(args["nstart"].tolist()))
        try:
            if eig:
                got = nx.eigenvector_centrality(nxg, max_iter=args["max_iter"], tol=args["tol"], nstart=nstart, weight="weight" if weighted else None)
            else:
                got = nx.katz_centrality(nxg, alpha=args["alpha"], beta=float(beta[0]) if beta.size == 1 else dict(enumerate(beta.tolist())),
                                         max_iter=args["max_iter"], tol=args["tol"], nstart=nstart, normalized=args["normalized"],
                                         weight="weight" if weighted else None)
        except nx.PowerIterationFailedConvergence:
            got = None
        assert (got is None) == (mine is None), name
        assert margin >= 1e-6, (name, margin)
        rtol = FLOOR
        values = np.zeros(0)
        if got is not None:
            values = np.array([got[v] for v in range(n)], dtype=np.float64)
            assert np.array_equal(values, np.array([mine[v] for v in range(n)])), name          # the restatement IS networkx's loop
            exact, _, _ = restated(nxg, kind, weighted, iterations, **loop)
            rtol = max(FLOOR, 16 * rtol_needed(np.array([exact[v] for v in range(n)]), values))
            worst_rtol = max(worst_rtol, rtol)
        worst_margin = min(worst_margin, margin)
        store[f"{name}/graph"] = np.array(g)
        store[f"{name}/kind"] = np.array(kind)
        store[f"{name}/max_iter"] = np.int64(args["max_iter"])
        store[f"{name}/tol"] = np.float64(args["tol"])
        store[f"{name}/alpha"] = np.float64(args["alpha"])
        store[f"{name}/beta"] = beta
        store[f"{name}/nstart"] = np.zeros(0) if args["nstart"] is None else args["nstart"]
        store[f"{name}/normalized"] = np.bool_(args["normalized"])
        store[f"{name}/weights"] = np.zeros(0) if weights is None else weights
        store[f"{name}/raised"] = np.bool_(got is None)
        store[f"{name}/values"] = values
        store[f"{name}/iterations"] = np.int64(iterations)
        store[f"{name}/margin"] = np.float64(margin)
        store[f"{name}/rtol"] = np.float64(rtol)
        names.append(name)
        print(f"{name:34s} n {n:5d} {'raised' if got is None else 'stops '} at {iterations:5d}  margin {margin:.2e}  rtol {rtol:.2e}")
    store["names"] = np.array(names)
    path = OUT / "spectral_centrality_vectors.npz"
    np.savez_compressed(path, **store)
    print(f"{len(names)} cases -> {path} ({path.stat().st_size} bytes); smallest margin {worst_margin:.2e}, largest rtol {worst_rtol:.2e}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
