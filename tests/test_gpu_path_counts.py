"""Shortest-path counts beyond the exact float64 range in the two betweenness kernels (csrc/pp_graph_paths.hip: k_graph_betweenness,
csrc/pp_paths.hip: k_temporal_betweenness), and the static search kernels with their grid set by the 1 GiB workspace budget.

The kernels count paths in float64; the static reference counts in Python ints, the temporal reference in float64 with an ``isnan``
guard on both ratios of its backward pass.  Three ranges:

* below 2**53 the counts are exact and the results bit-identical from run to run (tests/test_gpu_static_paths.py);
* from 2**53 to 2**1024 the counts round.  Every term is non-negative; a count carries at most (depth * in-degree) roundings and a
  dependency about as many again, below 10^3 * 2^-53 ~ 10^-13 relative on the inputs here (the CPU float64 forms sit 10^-15 and 10^-13
  from the exact answers, tests/test_path_counts_host.py), so the files' existing tolerances hold: static rtol = atol = 1e-10,
  temporal rtol 1e-10, atol 1e-9.  Bit-identity from run to run is NOT asserted here: atomic adds of inexact values land in any order;
* at 2**1024 a count is inf.  The static call raises OverflowError, for exactly the searched sources that have such a count — the
  chain of 1024 stages is served from its middle (2**512 paths) and refused from node 0.  Before the refusal the chain of 1024
  stages gave finite values, off by up to a third on 1023 of 1025 nodes (x / inf = 0), which no finiteness check of the result sees.
  The temporal call follows the reference's guard and stays equal to it, finite where it is finite; unguarded it gave NaN.

The inputs are built in tests/path_count_inputs.py; expected values come from tests/cpu_ops_static_paths.py (Python ints) and
oracle/temporal_paths.py."""
import functools

import numpy as np
import pytest
import torch

import cpu_ops_static_paths as ops
import path_count_inputs as pci
import pathpyg_amd as pp
from oracle import temporal_paths as tp
from pathpyg_amd import _dispatch, _hip
from pathpyg_amd.algorithms import centrality as ct
from pathpyg_amd.algorithms import shortest_paths as sp
from pathpyg_amd.algorithms import temporal as tm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(rtol=1e-10, atol=1e-10)
TOL_TEMPORAL = dict(rtol=1e-10, atol=1e-9)


def graph_of(ei, n):
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64).reshape(2, -1).to(DEV)
    return pp.Graph(pp.Data(edge_index=ei, num_nodes=n))


def temporal_graph_of(ei, t, n):
    return pp.TemporalGraph(pp.Data(edge_index=torch.from_numpy(ei).to(DEV), time=torch.from_numpy(t).to(DEV), num_nodes=n))


def check_betweenness(g, ei, n, sources):
    want, keys = ops.betweenness(ei, n, sources)
    bw = ct.betweenness_centrality(g, sources=sources)
    assert set(bw) == set(np.nonzero(keys)[0].tolist())
    np.testing.assert_allclose([bw[i] if i in bw else 0.0 for i in range(n)], want, **TOL)
    return want


def temporal_values(g, delta, n):
    bw = tm.temporal_betweenness_centrality(g, delta)
    return np.array([bw[i] for i in range(n)])


# ------------------------------------------------------------------ A1: irregular counts above 2**53
def test_static_betweenness_with_irregular_counts_above_2_to_the_53():
    ei, n, _ = pci.layered()
    largest = max(pci.exact_counts(ei, n, 0))
    assert 2 ** 100 <= largest < 2 ** 1000
    want = check_betweenness(graph_of(ei, n), ei, n, list(range(8)))      # the nodes of the layers 0 and 1
    assert want.max() > 1.0


def test_temporal_betweenness_with_irregular_counts_above_2_to_the_53():
    ei, t, n = pci.layered_stream()
    assert 2 ** 100 <= max(pci.exact_counts(ei, n, 0)) < 2 ** 1000        # the event paths of this stream are the static paths
    want = tp.temporal_betweenness_reference(torch.from_numpy(ei), torch.from_numpy(t), n, pci.LAYERED_DELTA)
    got = temporal_values(temporal_graph_of(ei, t, n), pci.LAYERED_DELTA, n)
    np.testing.assert_allclose(got, want, equal_nan=False, **TOL_TEMPORAL)


# ------------------------------------------------------------------ A2 - A4: the chain below, at and past 2**1024
@functools.lru_cache(maxsize=None)
def chain_temporal_reference(L):
    """The reference's values on the chain stream (seconds of Python per call: computed once per length)."""
    ei, t, n = pci.chain_stream(L)
    return tp.temporal_betweenness_reference(torch.from_numpy(ei), torch.from_numpy(t), n, pci.CHAIN_DELTA)


def test_static_chain_just_below_overflow():
    L = 1020
    ei, n = pci.chain(L)
    check_betweenness(graph_of(ei, n), ei, n, [0, 1, L // 2, L - 1])


@pytest.mark.parametrize("L", [1020, 1024, 1030])
def test_temporal_chain_below_at_and_past_overflow_equals_the_guarded_reference(L):
    ei, t, n = pci.chain_stream(L)
    want = chain_temporal_reference(L)
    assert np.isfinite(want).all()
    g = temporal_graph_of(ei, t, n)
    got = temporal_values(g, pci.CHAIN_DELTA, n)
    print(f"L = {L}: {int(np.isnan(got).sum())} NaN, {int((~np.isfinite(got)).sum())} non-finite of {n}; first {got[:4].tolist()}, last {got[-4:].tolist()}; "
          f"reference first {want[:4].tolist()}, last {want[-4:].tolist()}; max abs difference {np.nanmax(np.abs(got - want))}")
    np.testing.assert_allclose(got, want, equal_nan=False, **TOL_TEMPORAL)
    if L == 1030:
        assert tm.temporal_shortest_paths(g, pci.CHAIN_DELTA)[0][0, L] == L


@pytest.mark.parametrize("L", [1024, 1100])
def test_static_chain_at_and_past_overflow_is_refused_per_searched_source(L):
    ei, n = pci.chain(L)
    g = graph_of(ei, n)
    for sources in (None, [0]):
        with pytest.raises(OverflowError, match=r"2\*\*1024 or more shortest paths"):
            ct.betweenness_centrality(g, sources=sources)
    if L == 1024:                                                         # from the middle the largest count is 2**512: served, and exact
        assert max(pci.exact_counts(ei, n, L // 2)) == 2 ** (L // 2)
        check_betweenness(g, ei, n, [L // 2, L - 1])
    # the searches that count no paths are unaffected
    idx = np.arange(n)
    want = np.where(idx[None, :] >= idx[:, None], (idx[None, :] - idx[:, None]).astype(np.float64), np.inf)
    picks = [0, 1, L // 2, L]
    rows, pred_rows = ops.shortest_paths(ei, n, picks)
    assert np.array_equal(rows, want[picks])
    dist, pred = sp.shortest_paths_dijkstra(g)
    assert np.array_equal(dist, want) and dist[0, L] == L
    assert np.array_equal(pred[picks], pred_rows)
    assert sp.diameter(g) == ops.diameter(want) == np.inf and sp.avg_path_length(g) == ops.avg_path_length(want)
    assert list(ct.closeness_centrality(g).values()) == ops.closeness(want).tolist()


# ------------------------------------------------------------------ C: static grids set by the workspace budget
def component_rows(perm, n, sources):
    """Expected ``(dist, pred)`` int32 rows of the component graph for ``sources``: the restatement on ONE 8-node component, mapped
    through the permutation.  The predecessor is the largest node index among the tight ones AFTER the mapping."""
    local = pci.component_edges()
    ldist, _ = ops.shortest_paths(local, pci.COMPONENT)
    where = np.empty(n, dtype=np.int64)
    where[perm] = np.arange(n)                                            # position of a node id: 8 * component + local index
    dist = np.full((len(sources), n), -1, dtype=np.int32)
    pred = np.full((len(sources), n), ops.NO_PRED, dtype=np.int32)
    for i, s in enumerate(sources):
        base, j = where[s] // pci.COMPONENT * pci.COMPONENT, where[s] % pci.COMPONENT
        for k in range(pci.COMPONENT):
            if np.isfinite(ldist[j, k]):
                dist[i, perm[base + k]] = int(ldist[j, k])
                tight = [u for u, v in local.T.tolist() if v == k and np.isfinite(ldist[j, u]) and ldist[j, u] + 1 == ldist[j, k]]
                if k != j:
                    pred[i, perm[base + k]] = max(perm[base + u] for u in tight)
    return dist, pred


def test_bfs_grid_set_by_the_workspace_budget():
    n, k = 200_000, 700
    ei, perm = pci.component_paths(n, seed=41)
    sources = np.random.default_rng(43).choice(n, size=k, replace=False).tolist()
    parts = int(_hip.lib().pp_graph_bfs_parts(n, k))
    print(f"k_graph_bfs: {parts} slices for n = {n}, {k} sources")
    assert 1 < parts < k and parts < 2048
    g = graph_of(ei, n)
    # totals of all 700 searches: the sources past the grid are second sources of a workgroup
    ldist, _ = ops.shortest_paths(pci.component_edges(), pci.COMPONENT)
    where = np.empty(n, dtype=np.int64)
    where[perm] = np.arange(n)
    reach_in, dist_in = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    total, longest, no_path = 0, 0, 0
    late = 0
    for i, s in enumerate(sources):
        base, j = where[s] // pci.COMPONENT * pci.COMPONENT, where[s] % pci.COMPONENT
        hit = np.flatnonzero(np.isfinite(ldist[j]) & (np.arange(pci.COMPONENT) != j))
        reach_in[perm[base + hit]] += 1
        dist_in[perm[base + hit]] += ldist[j, hit].astype(np.int64)
        total += int(ldist[j, hit].sum())
        longest = max(longest, int(ldist[j, hit].max()) if hit.size else 0)
        no_path += n - 1 - hit.size
        late += i >= parts and hit.size > 0
    assert 2 * late >= k - parts, "the sources past the grid must reach something"
    got_reach, got_dist, got_totals = _dispatch.graph_path_totals(g, sources)
    assert got_reach == reach_in.tolist() and got_dist == dist_in.tolist()
    assert got_totals == [total, longest, no_path]
    # dense rows of the last 40 sources
    dist, pred = (x.cpu().numpy() for x in _dispatch.graph_shortest_paths(g, sources[-40:]))
    want_dist, want_pred = component_rows(perm, n, sources[-40:])
    assert np.array_equal(dist, want_dist) and np.array_equal(pred, want_pred)


def test_betweenness_grid_set_by_the_workspace_budget():
    n, k = 30_000, 1000
    ei, perm = pci.component_paths(n, seed=47)
    sources = np.random.default_rng(53).choice(n, size=k, replace=False).tolist()
    parts = int(_hip.lib().pp_graph_betweenness_parts(n, k))
    print(f"k_graph_betweenness: {parts} parts for n = {n}, {k} sources")
    assert 1 < parts < k and parts < 1024
    late, _ = ops.betweenness(ei, n, sources[parts:])
    assert 2 * int(np.count_nonzero(late)) >= k - parts, "the sources past the grid must carry weight"
    check_betweenness(graph_of(ei, n), ei, n, sources)
