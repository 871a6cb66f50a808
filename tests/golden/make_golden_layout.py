#!/usr/bin/env python3
"""Generate tests/golden/layout_vectors.npz from networkx's ``spring_layout`` and ``circular_layout`` and the reference's grid formula.

Needs networkx (3.4), scipy and numpy only, no checkout of the reference.  The reference's layouts see a graph through
``to_scipy_sparse_matrix(edge_index, edge_attr=weight)`` -> ``nx.from_scipy_sparse_array``: a coo matrix in stored order whose entries
become the edges of an undirected ``nx.Graph`` one after the other, a later entry of a pair overwriting an earlier one.  The graphs are
built that way here, from edge lists in a Graph's stored order (sorted by source, stable), so "the last stored edge of a pair wins" is
networkx's doing, not a restatement.  Every case gives all start
positions, so no random draw is involved.

    python tests/golden/make_golden_layout.py

The Fruchterman-Reingold map is chaotic: two float64 evaluations that sum in different orders differ by about 1e-16 of the layout's rms after
one iteration and about threefold more after every further one (1e-8 after 20, up to 3e-2 after 50).  So values are compared over short
horizons (1, 2, 3, 5 iterations), and a 50-iteration run is checked step by step from networkx's own states.

Content (``names`` are joined with ``/``):
  ``graphs`` and per graph ``graph/<g>/edge_index`` int32 [2, m], ``/n``, ``/weights`` ([0] = none, else one per stored edge) and ``/A``,
  networkx's dense adjacency, for the graphs with at most 64 nodes.
  ``cases`` (short horizons) and per case ``<c>/graph``, ``/pos0`` [n, 2], ``/k`` (NaN = None), ``/fixed`` (indices), ``/has_fixed``,
  ``/threshold``, ``/center``, ``/scale`` and ``/runs`` int [R, 2] = (iterations, 1 if rescaled with ``scale`` else 0 for ``scale=None``); per run
  ``<c>/run<r>/pos`` (networkx's result), ``/iterations`` (where it stopped) and ``/rtol``; ``<c>/margin``.
  ``trajectories`` and per trajectory the same arguments, ``/max_iterations``, ``/iterations`` (where networkx stopped), ``/dt``,
  ``/err_over_threshold`` (one per iteration run), ``/steps`` (iteration indices) and per step ``<t>/step<s>/before``, ``/t``, ``/after``,
  ``/rtol``: networkx's positions and temperature before that iteration and its positions after it; ``<t>/margin``.
  ``circular/<n>`` and ``grid/<n>``: the closed-form layouts, with ``circular_scale`` and ``circular_center``.

``margin``: the smallest relative distance of a compared quantity from the constant it is compared with, over all iterations of all runs of the
case — every pair distance from 0.01, every displacement length from 0.01, every ``err`` from ``threshold``.  Every case is asserted to
have margin >= 1e-6: rounding moves these quantities by about 1e-13 relative over the horizons used, so no correct implementation takes
another branch or stops at another iteration than networkx.  (The branch cases — all nodes on one point, two nodes 0.005 apart, a
displacement below 0.01 — sit far inside their branch and pass the same assertion.)

``rtol`` in the form of tests/tolerance.py, ``|got - want| <= rtol |want| + rtol rms(want)``: 16 times the largest rtol needed between
networkx's result and three other reference-side evaluations of the same case — the loop with exactly rounded sums (``math.fsum``; the
same restatement with plain sums is first checked bit for bit against networkx), the loop with the nodes permuted, and a loop that clips
the squared distance and sums repulsion and attraction apart — floor 2**-48.  Every rtol is asserted to be <= 1e-9: a case cannot buy a
loose bound.
"""
from __future__ import annotations

import math
import pathlib

import numpy as np

OUT = pathlib.Path(__file__).resolve().parent
FLOOR = 2.0 ** -48
RTOL_CAP = 1e-9
MARGIN_MIN = 1e-6
SHORT = (1, 2, 3, 5)
STEPS = (0, 10, 25, 40)


def nx_graph(nx, sp, edge_index, n, weights):
    data = np.ones(edge_index.shape[1]) if weights is None else weights
    return nx.from_scipy_sparse_array(sp.coo_matrix((data, (edge_index[0], edge_index[1])), shape=(n, n)))


def rescale(pos, scale, center):
    pos = pos.copy()
    pos -= pos.mean(axis=0)
    lim = np.abs(pos).max()
    if lim > 0:
        pos *= scale / lim
    return pos + center


def rel(x, c):
    return float(np.min(np.abs(np.asarray(x) / c - 1.0))) if np.size(x) else math.inf


def iterate(A, pos, k, fixed, iterations, threshold, t=None, dt=None, mode="plain", record=()):
    """networkx's dense loop in networkx's order of operations.  ``mode``: "plain" (its own numpy calls: the same bits), "fsum" (every sum
    exactly rounded), "clip2" (the squared distance is clipped; repulsion and attraction are summed apart).  Returns ``(pos, iterations run,
    margin, err / threshold per iteration, {iteration: (pos before, t before, pos after)}, dt)``."""
    pos = pos.astype(A.dtype)
    n = pos.shape[0]
    if t is None:
        t = max(max(pos.T[0]) - min(pos.T[0]), max(pos.T[1]) - min(pos.T[1])) * 0.1
        dt = t / (iterations + 1)
    margin, ratios, states, ran = math.inf, [], {}, 0
    off = ~np.eye(n, dtype=bool)
    for iteration in range(iterations):
        before = (pos.copy(), float(t)) if iteration in record else None
        delta = pos[:, np.newaxis, :] - pos[np.newaxis, :, :]
        if mode == "clip2":
            d2 = delta[:, :, 0] * delta[:, :, 0] + delta[:, :, 1] * delta[:, :, 1]
            distance = np.maximum(np.sqrt(d2), 0.01)
            displacement = k * k * np.einsum("ijk,ij->ik", delta, 1.0 / np.maximum(d2, 0.01 * 0.01)) - np.einsum("ijk,ij->ik", delta, A * distance) / k
        else:
            distance = np.linalg.norm(delta, axis=-1)
            margin = min(margin, rel(distance[off], 0.01))
            np.clip(distance, 0.01, None, out=distance)
            coef = k * k / distance**2 - A * distance / k
            if mode == "plain":
                displacement = np.einsum("ijk,ij->ik", delta, coef)
            else:
                terms = delta * coef[:, :, np.newaxis]
                displacement = np.array([[math.fsum(terms[i, :, 0]), math.fsum(terms[i, :, 1])] for i in range(n)])
        length = np.linalg.norm(displacement, axis=-1)
        margin = min(margin, rel(length, 0.01))
        length = np.where(length < 0.01, 0.1, length)
        delta_pos = np.einsum("ij,i->ij", displacement, t / length)
        if fixed is not None:
            delta_pos[fixed] = 0.0
        pos += delta_pos
        t -= dt
        ran += 1
        err = (math.sqrt(math.fsum((delta_pos * delta_pos).ravel())) if mode == "fsum" else np.linalg.norm(delta_pos)) / n
        ratios.append(err / threshold)
        margin = min(margin, abs(err / threshold - 1.0))
        if before is not None:
            states[iteration] = (*before, pos.copy())
        if err < threshold:
            break
    return pos, ran, margin, np.array(ratios), states, dt


def rtol_needed(got, want):
    rms = math.sqrt(float(np.mean(want * want))) if want.size else 0.0
    return float(np.max(np.abs(got - want) / (np.abs(want) + rms + 1e-300))) if want.size else 0.0


def spread(A, pos, k, fixed, iterations, threshold, want, ran, finish, rng, t=None, dt=None):
    """16 x the largest rtol needed between networkx's ``want`` and the other reference-side evaluations (which must stop where it did)."""
    n = pos.shape[0]
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    others = []
    for mode in ("fsum", "clip2"):
        got, r, *_ = iterate(A, pos, k, fixed, iterations, threshold, t, dt, mode)
        assert r == ran, (mode, r, ran)
        others.append(finish(got))
    got, r, *_ = iterate(A[perm][:, perm], pos[perm], k, None if fixed is None else inv[fixed], iterations, threshold, t, dt, "plain")
    assert r == ran, ("permuted", r, ran)
    others.append(finish(got[inv]))
    return max(FLOOR, 16.0 * max(rtol_needed(o, want) for o in others))


def random_edges(rng, n, m):
    return rng.integers(0, n, (2, m))


def graphs():
    """name -> (edge_index int64 [2, m], n, weights | None)"""
    rng = np.random.default_rng(7)
    out = {
        "n2": (np.array([[0], [1]]), 2, None),
        "path3": (np.array([[0, 1], [1, 2]]), 3, None),
    }
    for n in (63, 64, 65, 255, 256, 257):
        out[f"random_{n}"] = (random_edges(rng, n, 3 * n), n, None)
    out["random_1100"] = (random_edges(rng, 1100, 5500), 1100, None)
    hub = np.arange(1, 300)
    out["star_300"] = (np.concatenate([np.stack([np.zeros(299, dtype=np.int64), hub]), random_edges(rng, 300, 60)], axis=1), 300, None)
    out["isolated_40"] = (random_edges(rng, 30, 60), 40, None)                  # nodes 30 .. 39 have no edge
    loops = random_edges(rng, 30, 50)
    loops[1, ::5] = loops[0, ::5]
    out["loops_30"] = (loops, 30, rng.uniform(0.5, 2.0, 50))
    # parallel and antiparallel copies with different weights: the last stored copy of {0,1}, {1,2}, {3,4} decides; (2,2), (5,5) are loops
    multi = np.array([[0, 1, 0, 1, 2, 2, 3, 4, 3, 5, 4, 0, 2], [1, 0, 1, 2, 1, 2, 4, 3, 4, 5, 5, 5, 3]])
    out["multi_6"] = (multi, 6, np.array([1.0, 2.0, 3.0, 0.5, 4.0, 9.0, 1.5, 2.5, 0.25, 7.0, 1.0, 2.0, 1.25]))
    out["signed_50"] = (random_edges(rng, 50, 150), 50, rng.choice(np.array([-0.5, 0.0, 0.7, 2.0]), 150))
    out["random_80"] = (random_edges(rng, 80, 240), 80, None)
    out["random_100"] = (random_edges(rng, 100, 300), 100, None)
    out["path5"] = (np.array([[0, 1, 2, 3], [1, 2, 3, 4]]), 5, None)
    stored = {}
    for g, (ei, n, w) in out.items():                               # a Graph stores its edges sorted by source (stable), attributes alike
        ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
        order = np.argsort(ei[0], kind="stable")
        stored[g] = (ei[:, order], n, None if w is None else w[order])
    return stored


def short_cases(gs):
    """(case, graph, start positions, arguments, runs)"""
    rng = np.random.default_rng(11)
    full = [(i, s) for i in SHORT for s in (0, 1)]
    alternating = [(i, j % 2) for j, i in enumerate(SHORT)]
    for g in ("n2", "path3", "random_63", "random_64", "random_65", "random_255", "random_256", "random_257", "star_300", "isolated_40",
              "loops_30", "multi_6", "signed_50"):
        n = gs[g][1]
        yield g, g, rng.uniform(0.0, 1.0, (n, 2)), {}, full if n <= 65 else alternating
    yield "random_1100", "random_1100", rng.uniform(0.0, 1.0, (1100, 2)), {}, alternating
    yield "fixed_80", "random_80", rng.uniform(0.0, 1000.0, (80, 2)), dict(fixed=np.array([0, 5, 9])), [(i, 1) for i in SHORT]
    yield "center_scale_64", "random_64", rng.uniform(0.0, 1.0, (64, 2)), dict(center=np.array([3.0, -2.0]), scale=2.5, k=0.2), [(i, 1) for i in SHORT]
    pos = rng.uniform(0.0, 1.0, (100, 2))
    t0 = 0.1 * max(np.ptp(pos[:, 0]), np.ptp(pos[:, 1]))
    yield "stop_early_100", "random_100", pos, dict(threshold=0.9 * t0 / 10.0), [(5, 0), (5, 1)]    # err = t / sqrt(n): under it at the 2nd iteration
    # branch cases, far inside their branch
    yield "coincident_5", "path5", np.full((5, 2), 0.3), {}, [(3, 0), (3, 1)]                       # no force, t = 0: stops after one iteration
    yield "close_2", "n2", np.array([[0.5, 0.5], [0.503, 0.504]]), {}, [(1, 0), (3, 0), (3, 1)]      # 0.005 apart: the distance is clipped
    k2 = math.sqrt(0.5)
    yield "balanced_2", "n2", np.array([[0.0, 0.0], [k2 * 1.001, 0.0]]), {}, [(1, 0), (2, 0)]        # |disp| about 0.002 < 0.01: len = 0.1


def trajectory_cases(gs):
    rng = np.random.default_rng(13)
    for g in ("random_65", "random_1100"):              # (one below and one above a source tile; 17.6 kB per stored state at n = 1100)
        yield g, g, rng.uniform(0.0, 1.0, (gs[g][1], 2)), {}
    yield "fixed_80", "random_80", rng.uniform(0.0, 1000.0, (80, 2)), dict(fixed=np.array([0, 5, 9]))
    yield "stop_early_100", "random_100", rng.uniform(0.0, 1.0, (100, 2)), dict(threshold=5e-3)


def arguments(given, pos0, n):
    args = dict(k=None, fixed=None, threshold=1e-4, center=np.zeros(2), scale=1.0)
    args.update(given)
    k = args["k"]
    if k is None:                                                   # spring_layout's own default
        dom_size = max(float(pos0.max()), 0.0) or 1.0
        k = dom_size / np.sqrt(n) if args["fixed"] is not None else np.sqrt(1.0 / n)
    return args, k


def store_arguments(store, name, g, pos0, args):
    store[f"{name}/graph"] = np.array(g)
    store[f"{name}/pos0"] = pos0
    store[f"{name}/k"] = np.float64(np.nan if args["k"] is None else args["k"])
    store[f"{name}/has_fixed"] = np.bool_(args["fixed"] is not None)
    store[f"{name}/fixed"] = np.zeros(0, dtype=np.int64) if args["fixed"] is None else args["fixed"].astype(np.int64)
    store[f"{name}/threshold"] = np.float64(args["threshold"])
    store[f"{name}/center"] = args["center"]
    store[f"{name}/scale"] = np.float64(args["scale"])


def main() -> int:
    import networkx as nx
    import scipy.sparse as sp

    gs = graphs()
    store = {"graphs": np.array(list(gs))}
    dense = {}
    for g, (ei, n, w) in gs.items():
        G = nx_graph(nx, sp, ei, n, w)
        assert list(G) == list(range(n)), g
        dense[g] = (G, nx.to_numpy_array(G, weight="weight"))
        store[f"graph/{g}/edge_index"] = ei.astype(np.int32)
        store[f"graph/{g}/n"] = np.int64(n)
        store[f"graph/{g}/weights"] = np.zeros(0) if w is None else w
        if n <= 64:
            store[f"graph/{g}/A"] = dense[g][1]
    rng = np.random.default_rng(17)
    worst_margin, worst_rtol = math.inf, 0.0

    names = []
    for name, g, pos0, given, runs in short_cases(gs):
        G, A = dense[g]
        n = gs[g][1]
        args, k = arguments(given, pos0, n)
        fixed = args["fixed"]
        case_margin = math.inf
        store_arguments(store, name, g, pos0, args)
        store[f"{name}/runs"] = np.array(runs, dtype=np.int64)
        for r, (iterations, scaled) in enumerate(runs):
            rescales = bool(scaled) and fixed is None

            def finish(p):
                return rescale(p, args["scale"], args["center"]) if rescales else p

            mine, ran, margin, _, _, _ = iterate(A, pos0, k, fixed, iterations, args["threshold"])
            mine = finish(mine)
            if n < 500:                                             # spring_layout itself, through its dense routine
                got = nx.spring_layout(G, k=args["k"], pos=dict(enumerate(pos0)), fixed=None if fixed is None else fixed.tolist(),
                                       iterations=iterations, threshold=args["threshold"], weight="weight", scale=args["scale"] if scaled else None,
                                       center=args["center"])
                want = np.array([got[v] for v in range(n)])
            else:                                                   # beyond 500 nodes spring_layout turns to float32: the dense routine, directly
                want = finish(nx.drawing.layout._fruchterman_reingold(A, k, pos0.copy(), fixed, iterations, args["threshold"], 2, None))
            assert np.array_equal(mine, want), (name, iterations, scaled)      # the restatement IS networkx's loop
            rtol = spread(A, pos0, k, fixed, iterations, args["threshold"], want, ran, finish, rng)
            assert rtol <= RTOL_CAP, (name, iterations, rtol)
            store[f"{name}/run{r}/pos"] = want
            store[f"{name}/run{r}/iterations"] = np.int64(ran)
            store[f"{name}/run{r}/rtol"] = np.float64(rtol)
            case_margin = min(case_margin, margin)
            worst_rtol = max(worst_rtol, rtol)
            print(f"{name:18s} n {n:5d} iterations {iterations} -> {ran}  scaled {scaled}  margin {margin:.2e}  rtol {rtol:.2e}")
        assert case_margin >= MARGIN_MIN, (name, case_margin)
        store[f"{name}/margin"] = np.float64(case_margin)
        worst_margin = min(worst_margin, case_margin)
        names.append(name)
    store["cases"] = np.array(names)

    names = []
    for name, g, pos0, given in trajectory_cases(gs):
        G, A = dense[g]
        n = gs[g][1]
        args, k = arguments(given, pos0, n)
        fixed, threshold = args["fixed"], args["threshold"]
        final, ran, margin, ratios, states, dt = iterate(A, pos0, k, fixed, 50, threshold, record=range(50))
        want = nx.drawing.layout._fruchterman_reingold(A, k, pos0.copy(), fixed, 50, threshold, 2, None)
        assert np.array_equal(final, want), name
        steps = sorted({s for s in STEPS if s < ran} | {ran - 1})
        name = "trajectory_" + name
        store_arguments(store, name, g, pos0, args)
        store[f"{name}/max_iterations"] = np.int64(50)
        store[f"{name}/iterations"] = np.int64(ran)
        store[f"{name}/dt"] = np.float64(dt)
        store[f"{name}/err_over_threshold"] = ratios
        store[f"{name}/steps"] = np.array(steps, dtype=np.int64)
        for s in steps:
            before, t, after = states[s]
            again, one, step_margin, *_ = iterate(A, before, k, fixed, 1, threshold, t, dt)
            assert one == 1 and np.array_equal(again, after), (name, s)
            rtol = spread(A, before, k, fixed, 1, threshold, after, 1, lambda p: p, rng, t, dt)
            assert rtol <= RTOL_CAP, (name, s, rtol)
            store[f"{name}/step{s}/before"] = before
            store[f"{name}/step{s}/t"] = np.float64(t)
            store[f"{name}/step{s}/after"] = after
            store[f"{name}/step{s}/rtol"] = np.float64(rtol)
            worst_rtol = max(worst_rtol, rtol)
        assert margin >= MARGIN_MIN, (name, margin)
        store[f"{name}/margin"] = np.float64(margin)
        worst_margin = min(worst_margin, margin)
        names.append(name)
        print(f"{name:28s} n {n:5d} stops at {ran:2d}  steps {steps}  margin {margin:.2e}  last err / threshold {ratios[-1]:.3f}")
    store["trajectories"] = np.array(names)

    store["circular_scale"], store["circular_center"] = np.float64(2.5), np.array([1.0, -3.0])
    for n in (1, 2, 7):
        got = nx.circular_layout(range(n), scale=2.5, center=(1.0, -3.0))
        store[f"circular/{n}"] = np.array([got[v] for v in range(n)], dtype=np.float64)
    for n in (1, 5, 16):                                            # the reference's grid: side floor(sqrt(n)), width 1, rows downwards
        side = np.floor(np.sqrt(n))
        i = np.arange(0, n)
        store[f"grid/{n}"] = np.vstack(((i % side) * (1.0 / side), -np.floor(i / side) * (1.0 / side))).T

    path = OUT / "layout_vectors.npz"
    np.savez_compressed(path, **store)
    size = path.stat().st_size
    largest = max(p.stat().st_size for p in OUT.glob("*.npz") if p != path)
    assert size <= largest, (size, largest)
    print(f"{len(store['cases'])} cases, {len(names)} trajectories -> {path} ({size} bytes); smallest margin {worst_margin:.2e}, largest rtol {worst_rtol:.2e}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
