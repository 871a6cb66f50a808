"""The conditions that tests/test_gpu_path_counts.py and tests/test_gpu_temporal_paths.py lean on, checked on the CPU with the plain
restatements only (tests/cpu_ops_static_paths.py, oracle/temporal_paths.py; the product is not imported):

* the layered input's path counts are far above 2**53 and far below 2**1024, and the float64 forms of both recurrences still sit
  within 1e-12 of the exact ones there — the room the GPU tests' 1e-10 leaves to another summation order;
* the chain's float64 form equals the exact one up to counts of 2**1023 and is WRONG WITHOUT A NaN at 2**1024: ``x / inf`` is 0, so
  every value stays finite.  This is why the static search reports the count itself and a finiteness check of the result is no fix;
* the two budget streams keep the sources past the budget's grid busy, so a kernel that dropped them would be noticed.
"""
import numpy as np
import pytest
import torch

import cpu_ops_static_paths as ops
import path_count_inputs as pci
from oracle import lift
from oracle import temporal_paths as tp


def test_layered_counts_leave_the_exact_range_and_stay_finite():
    ei, n, _ = pci.layered()
    assert n == 284 and ei.shape[1] > 2 * (n - 4)
    largest = max(pci.exact_counts(ei, n, 0))
    assert 2 ** 100 <= largest < 2 ** 1000
    sources = list(range(8))
    want, keys = ops.betweenness(ei, n, sources)                      # Python ints
    got = ops.all_sources(ei, n, sources)                             # float64
    assert np.array_equal(got["keys"], keys) and want.max() > 1.0
    np.testing.assert_allclose(got["bw"], want, rtol=1e-12, atol=0.0)


def test_layered_stream_has_the_static_counts_and_its_float_forms_agree():
    ei, n, _ = pci.layered()
    sei, st, sn = pci.layered_stream()
    assert sn == n and (np.diff(st) >= 0).all()
    assert sorted(map(tuple, sei.T.tolist())) == sorted(map(tuple, ei.T.tolist()))
    # an event continues into every event out of its head node, all of them one layer on: the event graph is the static line graph
    pairs = lift.temporal_lift_sorted(torch.from_numpy(sei), torch.from_numpy(st), pci.LAYERED_DELTA, n)
    out = np.bincount(sei[0], minlength=n)
    assert pairs.size(1) == int(out[sei[1]].sum())
    ref = tp.temporal_betweenness_reference(torch.from_numpy(sei), torch.from_numpy(st), n, pci.LAYERED_DELTA)
    lev = tp.temporal_betweenness_levels(torch.from_numpy(sei), torch.from_numpy(st), n, pci.LAYERED_DELTA)
    assert np.isfinite(ref).all() and ref.max() > 1000.0
    # a source's own entry is (sum of dependencies) - (nodes reached) + 1, a difference of near-equal numbers: only its absolute error,
    # measured against the size of the values, means anything
    assert np.abs(lev - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("L", [1020, 1023])
def test_chain_float_form_is_exact_up_to_2_to_the_1023(L):
    ei, n = pci.chain(L)
    assert pci.exact_counts(ei, n, 0)[L] == 2 ** L
    sources = [0, 1, L // 2, L - 1]
    want, _ = ops.betweenness(ei, n, sources)
    got = ops.all_sources(ei, n, sources)["bw"]                       # powers of two: every count and every ratio is exact
    assert np.array_equal(got, want)


def test_chain_float_form_is_finite_and_wrong_at_2_to_the_1024():
    L = 1024
    ei, n = pci.chain(L)
    sources = [0, 1, L // 2, L - 1]
    want, _ = ops.betweenness(ei, n, sources)
    with np.errstate(over="ignore", invalid="ignore"):
        got = ops.all_sources(ei, n, sources)["bw"]
    assert np.isfinite(got).all()                                     # nothing to see for a finiteness check
    wrong = got != want
    assert wrong.sum() >= 1000 and (np.abs(got - want)[wrong] / want[wrong]).max() > 0.3
    # without the source whose counts overflow the same graph is served exactly: the largest count is 2**512
    sub = [L // 2, L - 1]
    assert max(pci.exact_counts(ei, n, L // 2)) == 2 ** (L // 2)
    assert np.array_equal(ops.all_sources(ei, n, sub)["bw"], ops.betweenness(ei, n, sub)[0])


def test_chain_stream_continues_into_the_next_stage_only():
    L = 40
    ei, t, n = pci.chain_stream(L)
    assert (np.diff(t) > 0).all()
    pairs = lift.temporal_lift_sorted(torch.from_numpy(ei), torch.from_numpy(t), pci.CHAIN_DELTA, n)
    assert pairs.size(1) == 4 * (L - 1)                               # both events of a stage into both events of the next
    assert bool((ei[0][pairs[1].numpy()] == ei[1][pairs[0].numpy()]).all())
    dist, _ = tp.temporal_shortest_paths_bfs(torch.from_numpy(ei), torch.from_numpy(t), n, pci.CHAIN_DELTA)
    assert dist[0, L] == L


def test_bfs_budget_stream_keeps_the_sources_past_the_grid_busy():
    seed, n, m, span, delta = pci.BFS_BUDGET_STREAM
    slices = pci.BFS_BUDGET_SLICES
    assert slices == 1988 and slices < n and slices < 2048
    ei, t = pci.random_stream(seed, n, m, span)
    dist, _ = tp.temporal_shortest_paths_bfs(torch.from_numpy(ei), torch.from_numpy(t), n, delta)
    far = [s for s in range(slices, n) if np.where(np.isfinite(dist[s]), dist[s], 0).max() >= 3]
    assert 2 * len(far) >= n - slices


def test_betweenness_budget_stream_keeps_the_sources_past_the_grid_busy():
    seed, n, m, span, delta = pci.BETWEENNESS_BUDGET_STREAM
    parts = pci.temporal_betweenness_parts(m, n)
    ei, t = pci.random_stream(seed, n, m, span)
    assert parts == 981 and parts < 1024 and parts < len(np.unique(ei[0]))
    want = tp.temporal_betweenness_reference(torch.from_numpy(ei), torch.from_numpy(t), n, delta)
    assert 2 * int(np.count_nonzero(want[parts:])) >= n - parts


def test_component_graph_has_two_tight_predecessors_and_counts_of_two():
    local = pci.component_edges()
    assert pci.exact_counts(local, pci.COMPONENT, 0) == [1, 1, 1, 2, 2, 2, 2, 2]
    dist, pred = ops.shortest_paths(local, pci.COMPONENT, [0])
    assert dist[0].tolist() == [0, 1, 1, 2, 3, 4, 5, 6] and pred[0, 3] == 2
    ei, perm = pci.component_paths(64, seed=1)
    assert ei.shape == (2, 64) and sorted(perm.tolist()) == list(range(64))
    full, _ = ops.shortest_paths(ei, 64, [int(perm[8])])              # local node 0 of component 1
    assert np.array_equal(np.flatnonzero(np.isfinite(full[0])), np.sort(perm[8:16]))
    assert full[0][perm[8:16]].tolist() == dist[0].tolist()
    assert pci.BUDGET // (8 * 200_000) == 671 and pci.graph_betweenness_parts(30_000, 1000) == 894
