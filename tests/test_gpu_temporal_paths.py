"""The temporal search kernels (csrc/pp_paths.hip: k_temporal_bfs, k_temporal_betweenness) through the public functions, at the smallest
shapes at which each of their mechanisms can fail: as many levels as events with a frontier of one, a frontier above one workgroup whose
events all have 300 successors and add into one node's count, predecessor ties between a tight and a later, longer arrival, equal
timestamps, an event graph without any pair, and two streams on which the 1 GiB workspace budget — not the node count, not the cap of
2048 / 1024 workgroups — sets the grid.

Held to the statement-by-statement restatements of the reference in oracle/temporal_paths.py.  Distances, predecessors (the oracle's
latest-tight-event rule) and closeness are exact: closeness adds the same float64 terms in the same order.  Betweenness: rtol 1e-10,
atol 1e-9, the bar of tests/test_gpu_api.py and tests/test_gpu_paths_many_sources.py — all path counts here are below 2**53 and exact,
every term is non-negative, and a dependency is a sum over (depth * successors) terms taken in another order than the reference's
stack: below 10^3 * 2^-53 ~ 10^-13 relative.  A source's own entry subtracts the number of reached nodes from such a sum of at most
a few thousand, which the absolute part covers."""
import numpy as np
import pytest
import torch

import path_count_inputs as pci
import pathpyg_amd as pp
from oracle import temporal_paths as tp
from pathpyg_amd import _dispatch, _hip
from pathpyg_amd.algorithms import temporal as tm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(rtol=1e-10, atol=1e-9)


def stream_of(ei, t, n):
    ei, t = torch.from_numpy(np.asarray(ei, dtype=np.int64).reshape(2, -1)), torch.from_numpy(np.asarray(t, dtype=np.int64))
    return ei, t, pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=n))


def check_stream(ei, t, n, delta, scipy_too=True):
    """Every public temporal search function on the time-sorted stream against the restatements.  Returns ``(dist, pred, bw)``."""
    ei, t, g = stream_of(ei, t, n)
    want_dist, want_pred = tp.temporal_shortest_paths_bfs(ei, t, n, delta)
    dist, pred = tm.temporal_shortest_paths(g, delta)
    assert dist.dtype == np.float64 and pred.dtype == np.int64 and dist.shape == pred.shape == (n, n)
    assert np.array_equal(dist, want_dist)
    if scipy_too:
        assert np.array_equal(dist, tp.temporal_shortest_paths_reference(ei, t, n, delta)[0])
    assert np.array_equal(pred, want_pred)                                # the source node of the latest tight event
    rows, cols = np.nonzero((pred != -1) & (pred != np.arange(n)[:, None]))
    assert np.isfinite(dist[rows, cols]).all()
    assert (dist[rows, pred[rows, cols]] + 1 == dist[rows, cols]).all()   # a tree: the predecessor is one event nearer
    assert (np.isinf(dist) == (pred == -1)).all() and (np.diag(dist) == 0).all() and (np.diag(pred) == np.arange(n)).all()
    bw = tm.temporal_betweenness_centrality(g, delta)
    bw = np.array([bw[g.mapping.to_id(i)] for i in range(n)])
    np.testing.assert_allclose(bw, tp.temporal_betweenness_reference(ei, t, n, delta), **TOL)
    cl = tm.temporal_closeness_centrality(g, delta)
    others = np.arange(n)
    assert cl == {g.mapping.to_id(i): float(sum((n - 1) / want_dist[others != i, i])) for i in range(n)}
    return dist, pred, bw


def test_time_respecting_chain_has_as_many_levels_as_events():
    m = 300
    ei = np.stack([np.arange(m), np.arange(1, m + 1)])
    dist, pred, bw = check_stream(ei, np.arange(m), m + 1, 1)
    assert (dist[0, 1:] == np.arange(1, m + 1)).all() and (pred[0, 1:] == np.arange(m)).all()
    assert np.isinf(dist[m, 0]) and bw[m] == 0.0 and bw[1] > 0.0


HUB_SIDE = 300


def hub_stream(t_in, t_out):
    """300 events leaf_i -> hub at ``t_in``, then 300 events hub -> out_j at ``t_out``: leaves 0 .. 299, hub 300, outs 301 .. 600."""
    leaves, hub, outs = np.arange(HUB_SIDE), HUB_SIDE, np.arange(HUB_SIDE + 1, 2 * HUB_SIDE + 1)
    ei = np.concatenate([np.stack([leaves, np.full(HUB_SIDE, hub)]), np.stack([np.full(HUB_SIDE, hub), outs])], axis=1)
    return ei, np.r_[np.full(HUB_SIDE, t_in), np.full(HUB_SIDE, t_out)], 2 * HUB_SIDE + 1


def test_hub_frontier_above_one_workgroup_and_300_adds_into_one_count():
    ei, t, n = hub_stream(0, 1)
    dist, pred, bw = check_stream(ei, t, n, 1)
    hub = HUB_SIDE
    assert (dist[:hub, hub + 1:] == 2).all() and (pred[:hub, hub + 1:] == hub).all() and (dist[hub, hub + 1:] == 1).all()
    assert bw[hub] == float(HUB_SIDE * HUB_SIDE) and not bw[:hub].any() and not bw[hub + 1:].any()


def test_hub_without_any_admissible_pair():
    ei, t, n = hub_stream(0, 5)
    ei_t, t_t, g = stream_of(ei, t, n)
    assert tuple(tm.lift_order_temporal(g, 4).shape) == (2, 0)
    dist, pred, bw = check_stream(ei, t, n, 4)
    want = np.full((n, n), np.inf)
    want[ei[0], ei[1]] = 1                                                # distances along single events only
    np.fill_diagonal(want, 0)
    assert np.array_equal(dist, want) and not bw.any()


def test_predecessor_ties_the_latest_tight_event_wins():
    a, b, c, x, d, y = range(6)
    events = [(a, b, 1), (a, c, 1), (a, x, 1), (b, d, 2), (x, y, 2), (c, d, 3), (y, d, 4), (d, a, 5)]
    ei = np.array([[u for u, _, _ in events], [v for _, v, _ in events]])
    dist, pred, _ = check_stream(ei, np.array([s for _, _, s in events]), 6, 5)
    assert dist[a, d] == 2 and pred[a, d] == c            # b -> d @ 2 and c -> d @ 3 are tight, the later one names the predecessor
    assert dist[a, y] == 2 and pred[a, y] == x            # (y -> d @ 4 is the latest event into d, but arrives at depth 3)
    assert dist[a, a] == 0 and pred[a, a] == a            # d -> a @ 5 returns to the source: the diagonal stays
    assert dist[b, a] == 2 and pred[b, a] == d


def test_equal_timestamps_never_chain():
    a, b, c = range(3)
    dist, _, _ = check_stream([[a, b], [b, c]], [3, 3], 3, 10)
    assert np.isinf(dist[a, c]) and dist[a, b] == 1 and dist[b, c] == 1
    dist, pred, _ = check_stream([[a, b], [b, c]], [3, 4], 3, 10)
    assert dist[a, c] == 2 and pred[a, c] == b


def test_bfs_grid_set_by_the_workspace_budget():
    seed, n, m, span, delta = pci.BFS_BUDGET_STREAM
    slices = _hip.lib().pp_temporal_bfs_ws_bytes(m, n) // (12 * m)          # 12 m bytes of state per workgroup
    print(f"k_temporal_bfs: {slices} slices for m = {m}, n = {n}")
    assert 1 < slices < 2048 and slices < n
    ei, t = pci.random_stream(seed, n, m, span)
    ei, t, g = stream_of(ei, t, n)
    want_dist, want_pred = tp.temporal_shortest_paths_bfs(ei, t, n, delta)
    far = [s for s in range(slices, n) if np.where(np.isfinite(want_dist[s]), want_dist[s], 0).max() >= 3]
    print(f"sources past the grid that reach distance >= 3: {len(far)} of {n - slices}")
    assert 2 * len(far) >= n - slices, "the sources past the grid must reach beyond their neighbours"
    dist, pred = tm.temporal_shortest_paths(g, delta)
    assert np.array_equal(dist, want_dist) and np.array_equal(pred, want_pred)


def test_betweenness_grid_set_by_the_workspace_budget():
    seed, n, m, span, delta = pci.BETWEENNESS_BUDGET_STREAM
    parts = int(_hip.lib().pp_temporal_betweenness_parts(m, n))
    ei, t = pci.random_stream(seed, n, m, span)
    print(f"k_temporal_betweenness: {parts} parts for m = {m}, n = {n}")
    assert 1 < parts < 1024 and parts < len(np.unique(ei[0]))
    ei, t = torch.from_numpy(ei), torch.from_numpy(t)
    want = tp.temporal_betweenness_reference(ei, t, n, delta)
    busy = int(np.count_nonzero(want[parts:]))
    print(f"nodes past the grid with a non-zero centrality: {busy} of {n - parts}")
    assert 2 * busy >= n - parts, "the sources past the grid must carry weight"
    got = _dispatch.temporal_betweenness(ei.to(DEV), t.to(DEV), n, delta).cpu().numpy()
    np.testing.assert_allclose(got, want, **TOL)
