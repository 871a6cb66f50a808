"""Host side of the distributions and PageRank feature: the refusals of ``pagerank``, ``personalized_pagerank``, ``RandomWalk.evolve`` and
``RandomWalk.stationary_distribution`` that are raised before any device work (argument forms and values, sizes by arithmetic), and the
restatements of tests/cpu_ops_diffusion.py held to closed forms (a 2-cycle, a star, a sink).  No GPU is touched."""
import math

import numpy as np
import pytest
import torch

import cpu_ops_diffusion as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip, _lib
from pathpyg_amd.algorithms import centrality, ranking


def host_graph(edges, n, ids=None, **attrs):
    """A row-sorted host Graph made without device work (num_nodes given, rows known to be sorted)."""
    ei = torch.tensor(sorted(edges), dtype=torch.int64).reshape(-1, 2).t().contiguous()
    return pp.Graph(pp.Data(edge_index=ei, num_nodes=n, **attrs), mapping=None if ids is None else pp.IndexMap(ids), _row_sorted=True)


TRIANGLE = [(0, 1), (1, 2), (2, 0)]


# ------------------------------------------------------------------ the package: refusals before any device work
def test_exports():
    assert pp.algorithms.pagerank is ranking.pagerank and pp.algorithms.personalized_pagerank is ranking.personalized_pagerank
    assert hasattr(pp.processes.RandomWalk, "evolve") and hasattr(pp.processes.RandomWalk, "stationary_distribution")
    assert hasattr(pp.processes.RandomWalk, "first_order") and pp.processes.Evolution is pp.processes.random_walk.Evolution
    assert hasattr(pp.MultiOrderModel, "pagerank") and hasattr(pp.MultiOrderModel, "stationary_distribution")


def test_pagerank_null_graph():
    g = pp.Graph(pp.Data(edge_index=torch.empty((2, 0), dtype=torch.int64), num_nodes=0), _row_sorted=True)
    assert ranking.pagerank(g) == {}
    assert ranking.pagerank(g, return_tensor=True).shape == (0,)


@pytest.mark.parametrize("alpha", [-0.1, 1.5, float("nan"), float("inf")])
def test_pagerank_refuses_alpha(alpha):
    g = host_graph(TRIANGLE, 3)
    with pytest.raises(ValueError, match="alpha"):
        ranking.pagerank(g, alpha=alpha)
    with pytest.raises(ValueError, match="alpha"):
        ranking.personalized_pagerank(g, torch.tensor([0]), alpha=alpha)


@pytest.mark.parametrize("name", ["personalization", "nstart", "dangling"])
def test_pagerank_refuses_vectors(name):
    g = host_graph(TRIANGLE, 3)
    for bad in ([1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], [0.0, 0.0, 0.0], {0: -1.0}, {0: 0.0}, {}):
        value = bad if isinstance(bad, dict) else np.array(bad)
        with pytest.raises(ValueError, match=name):
            ranking.pagerank(g, **{name: value})
    for key in (3, -1, "a", 0.5, True):
        with pytest.raises(ValueError, match="no node index"):
            ranking.pagerank(g, **{name: {key: 1.0}})
    with pytest.raises(ValueError):
        ranking.pagerank(g, **{name: np.ones(4)})            # one entry per node
    with pytest.raises(TypeError):
        ranking.pagerank(g, **{name: "uniform"})


def test_pagerank_refuses_other_arguments():
    g = host_graph(TRIANGLE, 3, edge_weight=torch.ones(3))
    with pytest.raises(ValueError, match="max_iter"):
        ranking.pagerank(g, max_iter=0)
    with pytest.raises(KeyError):
        ranking.pagerank(g, weight="edge_nothing")
    with pytest.raises(KeyError):
        ranking.personalized_pagerank(g, torch.tensor([0]), weight="edge_nothing")


def test_personalized_pagerank_refuses_seeds():
    g = host_graph(TRIANGLE, 3)
    for bad in (torch.tensor([3]), torch.tensor([-1]), torch.tensor([[0, 1]]), torch.tensor([True, False, True]), "a", 5):
        with pytest.raises(ValueError, match="seeds"):
            ranking.personalized_pagerank(g, bad)
    with pytest.raises(ValueError):
        ranking.personalized_pagerank(g, torch.ones(4, 2))                       # [n, B] has n rows
    with pytest.raises(ValueError):
        ranking.personalized_pagerank(g, torch.ones(3))                          # a float vector is no matrix
    with pytest.raises(ValueError, match="column 1"):
        ranking.personalized_pagerank(g, torch.tensor([[1.0, 0.0], [0.0, 0.0], [1.0, 0.0]]))
    with pytest.raises(ValueError, match="seeds"):
        ranking.personalized_pagerank(g, torch.tensor([[1.0, -1.0], [0.0, 1.0], [1.0, 1.0]]))
    ids = host_graph(TRIANGLE, 3, ids=["a", "b", "c"])
    with pytest.raises(ValueError, match="unknown node id"):
        ranking.personalized_pagerank(ids, ["a", "z"])


def test_failed_convergence_lists_columns():
    e = centrality.PowerIterationFailedConvergence(7, [2, 5])
    assert e.max_iter == 7 and e.columns == [2, 5] and "[2, 5]" in str(e)
    e = centrality.PowerIterationFailedConvergence(7)
    assert e.columns is None and str(e) == "power iteration failed to converge within 7 iterations"


def test_evolve_refusals():
    rw = pp.processes.RandomWalk(host_graph(TRIANGLE, 3))
    for steps in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="steps"):
            rw.evolve("weighted", steps)
    for lazy in (-0.1, 1.1, float("nan"), "half", True):
        with pytest.raises(ValueError, match="lazy"):
            rw.evolve("weighted", 1, lazy=lazy)
        with pytest.raises(ValueError, match="lazy"):
            rw.stationary_distribution(lazy=lazy)
    for start in ("somewhere", 5, None, torch.tensor([[0, 1]]), torch.tensor([True]), torch.ones(3, 2, 2), [], torch.empty(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="start"):
            rw.evolve(start, 1)
    for start in (torch.tensor([3]), torch.tensor([-1]), [0, 3]):
        with pytest.raises(ValueError, match="start"):
            rw.evolve(start, 1)
    for start in (torch.tensor([1.0, -1.0, 1.0]), torch.tensor([1.0, float("nan"), 1.0]), torch.tensor([1.0, float("inf"), 0.0]), torch.zeros(3),
                  torch.ones(4), torch.tensor([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])):
        with pytest.raises(ValueError, match="start"):
            rw.evolve(start, 1)
        with pytest.raises(ValueError, match="nstart"):
            rw.stationary_distribution(nstart=start)
    for target in ("uniform", torch.ones(3, 1), torch.ones(4), torch.zeros(3), torch.tensor([0, 1, 2]), [1.0, 1.0, 1.0], torch.tensor([1.0, -1.0, 1.0])):
        with pytest.raises(ValueError, match="target"):
            rw.evolve(torch.tensor([0]), 1, target=target)
    with pytest.raises(ValueError, match="max_iter"):
        rw.stationary_distribution(max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        rw.stationary_distribution(tol=0.0)
    with pytest.raises(ValueError, match="tol"):
        rw.stationary_distribution(tol=float("nan"))
    empty = pp.processes.RandomWalk(pp.Graph(pp.Data(edge_index=torch.empty((2, 0), dtype=torch.int64), num_nodes=0), _row_sorted=True))
    with pytest.raises(ValueError, match="no nodes"):
        empty.evolve("weighted", 1)
    with pytest.raises(ValueError):
        rw.first_order(torch.ones(4))
    model = pp.MultiOrderModel()
    with pytest.raises(ValueError, match="no layer"):
        model.pagerank(2)
    with pytest.raises(ValueError, match="no layer"):
        model.stationary_distribution(2)


def test_size_refusals_are_arithmetic():
    """n, nnz < 2^31 - 1, a padded width that is a power of two up to 64, and n * width * 8 * kept below 2^47 bytes: refused from the
    arguments, nothing is allocated."""
    limit = (1 << 31) - 1
    _hip.diffusion_check_sizes(limit - 1, limit - 1, 64, 2)
    _hip.diffusion_check_sizes(1 << 20, 10, 64, 1 << 18)                            # 2^20 * 64 * 8 * 2^18 = 2^47: the last that fits
    for args in ((limit, 10, 1, 2), (10, limit, 1, 2), (1 << 20, 10, 64, (1 << 18) + 1), (1 << 30, 10, 64, 1 << 9), (3, 3, 1, 1 << 62)):
        with pytest.raises(_lib.HipError, match="-4"):
            _hip.diffusion_check_sizes(*args)
    for args in ((-1, 1, 1, 2), (1, -1, 1, 2), (1, 1, 0, 2), (1, 1, 3, 2), (1, 1, 128, 2), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            _hip.diffusion_check_sizes(*args)
    assert [_hip.diffusion_width(b) for b in (1, 2, 3, 16, 17, 64)] == [1, 2, 4, 16, 32, 64]
    with pytest.raises(ValueError):
        _hip.diffusion_width(65)
    rw = pp.processes.RandomWalk(host_graph(TRIANGLE, 3))
    with pytest.raises(_lib.HipError, match="-4"):
        rw.evolve("weighted", 1 << 62, keep_all=True)                              # 3 * 8 * 2^62 bytes


# ------------------------------------------------------------------ the restatements against closed forms
def test_merged_entries():
    ei = np.array([[0, 0, 1, 0, 2], [1, 1, 0, 2, 2]])
    src, dst, w = ops.merged(ei, 3)
    assert src.tolist() == [0, 0, 1, 2] and dst.tolist() == [1, 2, 0, 2] and w.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert ops.merged(ei, 3, count_stored=True)[2].tolist() == [2.0, 1.0, 1.0, 1.0]
    assert ops.merged(ei, 3, weights=np.array([0.5, 0.25, 2.0, 1.0, 0.0]))[2].tolist() == [0.75, 1.0, 2.0, 0.0]
    T, prob, dangling = ops.table(*ops.merged(ei, 3, weights=np.array([0.5, 0.25, 2.0, 1.0, 0.0])), 3)
    assert T.tolist() == [1.75, 2.0, 0.0] and prob.tolist() == [0.75 / 1.75, 1.0 / 1.75, 1.0, 0.0] and dangling.tolist() == [False, False, True]


def test_two_cycle():
    """0 <-> 1: the mass swaps sides at lazy 0 (period 2: no convergence from one side), and halves its distance at lazy 0.5."""
    src, dst, w = ops.merged(np.array([[0, 1], [1, 0]]), 2)
    T, prob, dangling = ops.table(src, dst, w, 2)
    exact = ops.evolve_exact([1.0, 0.0], src, dst, prob, dangling, 2, 4)
    assert exact.tolist() == [[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0]]
    M = ops.dense_matrix(src, dst, prob, dangling, 2)
    assert np.array_equal(ops.evolve_numpy([1.0, 0.0], M, 4), exact)
    assert ops.stationary_numpy([1.0, 0.0], M, 1e-12, 50) == (None, 50)
    assert ops.stationary_numpy([0.5, 0.5], M, 1e-12, 50)[1] == 1
    lazy = ops.evolve_exact([1.0, 0.0], src, dst, prob, dangling, 2, 3, lazy=0.5)
    assert lazy.tolist() == [[1.0, 0.0], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5]]
    x, it = ops.stationary_numpy([1.0, 0.0], ops.dense_matrix(src, dst, prob, dangling, 2, lazy=0.5), 1e-12, 50)
    assert x.tolist() == [0.5, 0.5] and it == 2
    assert ops.tvd(exact, [0.5, 0.5]).tolist() == [0.5] * 5


def test_star():
    """An undirected star with k leaves: from the centre the mass alternates; the stationary distribution is degree / 2k; PageRank of the
    centre in closed form."""
    k = 4
    ei = np.array([[0] * k + list(range(1, k + 1)), list(range(1, k + 1)) + [0] * k])
    src, dst, w = ops.merged(ei, k + 1)
    T, prob, dangling = ops.table(src, dst, w, k + 1)
    assert T.tolist() == [4.0, 1.0, 1.0, 1.0, 1.0] and not dangling.any()
    exact = ops.evolve_exact([1.0] + [0.0] * k, src, dst, prob, dangling, k + 1, 2)
    assert exact[1].tolist() == [0.0] + [0.25] * k and exact[2].tolist() == [1.0] + [0.0] * k
    M = ops.dense_matrix(src, dst, prob, dangling, k + 1, lazy=0.5)
    pi = ops.dominant_left_eigenvector(M)
    assert np.allclose(pi, T / T.sum(), rtol=0, atol=1e-15)
    x, _ = ops.stationary_numpy(T / T.sum(), M, 1e-12, 10)
    assert np.array_equal(x, T / T.sum())
    # PageRank: c = alpha * (1 - c) + (1 - alpha) / n  =>  c = (alpha + (1 - alpha) / n) / (1 + alpha)
    alpha, n = 0.85, k + 1
    uniform = np.repeat(1.0 / n, n)
    got = ops.pagerank_exact(uniform, uniform, uniform, src, dst, prob, dangling, n, alpha, 400)
    centre = (alpha + (1 - alpha) / n) / (1 + alpha)
    assert abs(got[0] - centre) < 1e-15 and np.allclose(got[1:], (1 - centre) / k, rtol=0, atol=1e-15) and abs(got.sum() - 1) < 1e-15


def test_sink():
    """0 -> 1 -> 2, 2 a sink: the mass arrives and stays; PageRank spreads the sink's mass by the dangling weights."""
    src, dst, w = ops.merged(np.array([[0, 1], [1, 2]]), 3)
    T, prob, dangling = ops.table(src, dst, w, 3)
    assert dangling.tolist() == [False, False, True]
    exact = ops.evolve_exact([1.0, 0.0, 0.0], src, dst, prob, dangling, 3, 4)
    assert exact.tolist() == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]
    assert ops.tvd(exact, [0.0, 0.0, 1.0]).tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    M = ops.dense_matrix(src, dst, prob, dangling, 3)
    assert np.array_equal(ops.evolve_numpy(np.eye(3), M, 2)[2], np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]))    # [n, B]: column c started at c
    uniform = np.repeat(1.0 / 3, 3)
    one = ops.pagerank_exact(uniform, uniform, uniform, src, dst, prob, dangling, 3, 0.5, 1)
    # x0 = 1/3 each, D = 1/3: x'[0] = 0.5 * (0 + 1/9) + 1/6, x'[1] = x'[2] = 0.5 * (1/3 + 1/9) + 1/6
    assert np.allclose(one, [0.5 / 9 + 1 / 6, 0.5 * (1 / 3 + 1 / 9) + 1 / 6, 0.5 * (1 / 3 + 1 / 9) + 1 / 6], rtol=0, atol=1e-16)
    assert math.isclose(one.sum(), 1.0, abs_tol=1e-15)
    assert ops.rtol_needed(np.array([1.0, 2.0]), np.array([1.0, 2.0])) == 0.0
