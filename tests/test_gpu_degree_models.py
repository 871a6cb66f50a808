"""The degree-sequence models of pathpyg_amd.algorithms.generative_models on the device (k_mr_* and k_eg_check of csrc/pp_random_graphs.hip):
the Erdös-Gallai test against the reference's recorded answers, and every sampled edge set compared EXACTLY, with its number of repair
rounds, with the plain restatement (tests/cpu_ops_degree_models.py) at the smallest sequences at which each rule can go wrong — one edge,
nothing to repair, loops and duplicates together with blocked claims, zero-degree nodes, a single realisation (rejected and plateau
swaps), a star (loops only), tens of swaps in a round, and 3000 edges over a grid that needs several grid-stride passes."""
import functools
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_degree_models as ops
from cpu_ops_generative import graph_pairs
from pathpyg_amd import _hip
from pathpyg_amd.algorithms import generative_models as gm

pytestmark = pytest.mark.gpu

GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "degree_models_vectors.npz", allow_pickle=False)
SEQUENCES = [[1, 1], [1, 1, 1, 1], [2, 2, 2], [0, 2, 2, 0, 2, 0], [2, 2, 3, 2, 3], [2, 4, 3, 4, 3], [7] * 8, [15] + [1] * 15, [40, 40] + [2] * 78]
SEEDS = range(8)
ROUND_CAP = 256


@functools.lru_cache(maxsize=None)
def restated(seq: tuple, seed: int, multiedge: bool = False, relax: bool = False):
    return ops.molloy_reed(list(seq), seed, multiedge, relax)


def golden_cases():
    ptr, values = GOLDEN["eg/ptr"].tolist(), GOLDEN["eg/values"].tolist()
    return [(values[ptr[i]:ptr[i + 1]], bool(g)) for i, g in enumerate(GOLDEN["eg/graphic"].tolist())]


def stored_degrees(g, n):
    deg = [0] * n
    for u, _ in graph_pairs(g):
        deg[u] += 1
    return deg


def check_graph(g, n):
    pairs = graph_pairs(g)
    assert pairs == sorted(pairs) and g.n == n and g.mapping.num_ids() == n and g.is_undirected()
    assert g.data.edge_index.dtype == torch.int64 and getattr(g.data.edge_index, "is_undirected", False)
    stored = set(pairs)
    assert all(u != w and (w, u) in stored for u, w in pairs)
    return pairs


# ------------------------------------------------------------------ Erdös-Gallai
def test_erdos_gallai_fixture_host_and_device_input():
    """2016 sequences with n >= 2; every eighth one also as a device tensor and as float64 (the rest as lists: one code path less each)."""
    for i, (seq, graphic) in enumerate(golden_cases()):
        if len(seq) < 2:
            continue
        assert gm.is_graphic_erdos_gallai(seq) is graphic, seq
        if i % 8 == 0 or len(seq) == 200:
            assert gm.is_graphic_erdos_gallai(torch.tensor(seq, device="cuda")) is graphic, seq
            assert gm.is_graphic_erdos_gallai(np.array(seq, dtype=np.float64)) is graphic, seq
            assert gm.is_graphic_erdos_gallai(torch.tensor(seq, dtype=torch.int32)) is graphic, seq


def test_erdos_gallai_corners():
    assert gm.is_graphic_erdos_gallai([2]) is False and gm.is_graphic_erdos_gallai([0]) is True and gm.is_graphic_erdos_gallai([]) is True
    assert gm.is_graphic_erdos_gallai([1, -1]) is False and gm.is_graphic_erdos_gallai([2, 2, -2, 2]) is False            # negative entries
    assert gm.is_graphic_erdos_gallai([1, 1, 1]) is False and gm.is_graphic_erdos_gallai([2, 2, 1]) is False              # odd sums
    assert gm.is_graphic_erdos_gallai([1 << 62, 1 << 62]) is False and gm.is_graphic_erdos_gallai([1e30, 1e30]) is False
    for bad in ([1.0, 0.5, 0.5], [1.0, float("nan")], torch.tensor([1.0, float("inf")], device="cuda")):
        with pytest.raises(ValueError):
            gm.is_graphic_erdos_gallai(bad)


def test_erdos_gallai_many_workgroups():
    """2200 values of r under an 8-workgroup grid of 2048 lanes (a second grid-stride pass).  A clique of 1100 nodes joined to each of 1100
    further nodes is a graph whose sequence meets the condition with equality at r = 1100, a lane of the second pass; with two of the
    further nodes one stub short the condition fails at r = 1100 and 1101 and nowhere else, with an edge between them it holds again."""
    split = [2199] * 1100 + [1100] * 1100
    short = [2199] * 1100 + [1100] * 1098 + [1099, 1099]
    joined = [2199] * 1100 + [1100] * 1098 + [1101, 1101]
    assert ops.erdos_gallai(split) and not ops.erdos_gallai(short) and ops.erdos_gallai(joined)
    rng = np.random.default_rng(5)
    for share in (1000, 1):
        with _hip.launch_share(share):
            for seq, graphic in ((split, True), (short, False), (joined, True), ([6] * 2200, True)):
                assert gm.is_graphic_erdos_gallai(rng.permutation(seq)) is graphic


# ------------------------------------------------------------------ the sampler against its restatement
@pytest.mark.parametrize("seq", SEQUENCES, ids=lambda s: f"n{len(s)}max{max(s)}")
def test_molloy_reed_equals_restatement(seq):
    for seed in SEEDS:
        expect, rounds = restated(tuple(seq), seed)
        assert rounds <= ROUND_CAP
        g = gm.molloy_reed(seq, seed=seed)
        assert check_graph(g, len(seq)) == expect, seed
        assert gm.last_repair_rounds == rounds and gm.last_seed == seed
        assert stored_degrees(g, len(seq)) == seq and g.m == sum(seq) // 2 and g.nodes == list(range(len(seq)))
        assert g.data.edge_index.is_cuda
    if seq == [7] * 8:
        assert expect == [(u, w) for u in range(8) for w in range(8) if u != w]


def test_molloy_reed_grid_independence():
    """6000 stubs and 3000 edges: under ``launch_share(1)`` the 8 workgroups take a second (stubs: a third) grid-stride pass in every kernel."""
    seq = [6] * 1000
    expect, rounds = restated(tuple(seq), 11)
    results = []
    for share in (1, 1000):
        with _hip.launch_share(share):
            g = gm.molloy_reed(seq, seed=11)
            assert _hip.last_persistent_grid() >= 8
            results.append(check_graph(g, 1000))
            assert gm.last_repair_rounds == rounds
    assert results[0] == results[1] == expect and rounds >= 1
    assert stored_degrees(g, 1000) == seq
    other = graph_pairs(gm.molloy_reed(seq, seed=12))
    assert other != expect and other == restated(tuple(seq), 12)[0]                                     # another seed, another graph
    assert graph_pairs(gm.molloy_reed(torch.tensor(seq, device="cuda"), seed=11)) == expect                # device input; the same call twice


def test_molloy_reed_multiedge():
    seq = [4, 4, 2, 2, 2, 2]
    parallel = 0
    for seed in SEEDS:
        expect, rounds = restated(tuple(seq), seed, True)
        g = gm.molloy_reed(seq, multiedge=True, seed=seed)
        pairs = graph_pairs(g)
        assert pairs == expect and gm.last_repair_rounds == rounds
        assert all(u != w for u, w in pairs) and stored_degrees(g, 6) == seq and g.is_undirected() and g.n == 6
        parallel += len(pairs) - len(set(pairs))
    assert parallel > 0


def test_molloy_reed_relax():
    fewer = 0
    for seq in ([4, 4, 2, 2, 2, 2], [2, 2, 2], [7] * 8):
        for seed in SEEDS:
            expect, _ = restated(tuple(seq), seed, False, True)
            g = gm.molloy_reed(seq, relax=True, seed=seed)
            assert gm.last_repair_rounds == 0
            if not expect:                                                                                  # three loops: nothing is left
                assert g.n == 0 and g.m == 0
                continue
            assert check_graph(g, len(seq)) == expect
            fewer += g.m < sum(seq) // 2
    assert fewer > 0


def test_molloy_reed_refusals():
    for seq in ([1, 0], [2, 2, 6, 2, 3]):
        for kw in ({}, {"multiedge": True}, {"relax": True}):
            with pytest.raises(ValueError, match="not graphic"):
                gm.molloy_reed(seq, seed=1, **kw)
    g = gm.molloy_reed([0, 0, 0], seed=1)
    assert g.n == 0 and g.m == 0 and gm.last_repair_rounds == 0


def test_first_matching_uniform_on_device():
    """Over seeds 0 .. 599 each of the three perfect matchings of [1, 1, 1, 1] appears 200 +- 5 sigma times; the counts are the stream's."""
    counts = {}
    for seed in range(600):
        key = tuple(graph_pairs(gm.molloy_reed([1, 1, 1, 1], seed=seed, device="cpu")))
        counts[key] = counts.get(key, 0) + 1
    assert len(counts) == 3 and all(142 <= c <= 258 for c in counts.values()), counts
    assert sorted(counts.values()) == [191, 202, 207]


# ------------------------------------------------------------------ the functions built on it
def test_k_regular_random():
    g = gm.k_regular_random(3, 10, seed=4)
    assert stored_degrees(g, 10) == [3] * 10 and g.nodes == list(range(10)) and check_graph(g, 10) == restated((3,) * 10, 4)[0]
    ids = [f"v{i}" for i in range(10)]
    h = gm.k_regular_random(3, node_ids=ids, seed=4)
    assert h.nodes == ids and graph_pairs(h) == graph_pairs(g)
    with pytest.raises(ValueError, match="not graphic"):
        gm.k_regular_random(3, 5)


def test_molloy_reed_randomize():
    g = gm.erdos_renyi_gnm(200, 600, seed=3)
    r = gm.molloy_reed_randomize(g, seed=5)
    assert r.is_undirected() and r.n == 200 and r.m == 600 and r.nodes == g.nodes and r.data.edge_index.is_cuda
    assert r.degrees() == g.degrees() and graph_pairs(r) != graph_pairs(g)
    degrees = g.degrees(mode="in", return_tensor=True).tolist()
    assert check_graph(r, 200) == restated(tuple(degrees), 5)[0]
    host = gm.molloy_reed_randomize(g, seed=5, device="cpu")
    assert not host.data.edge_index.is_cuda and graph_pairs(host) == graph_pairs(r) and host.nodes == g.nodes
    assert graph_pairs(gm.molloy_reed_randomize(host, seed=5)) == graph_pairs(r)                           # a host graph is staged
    with pytest.raises(NotImplementedError):
        gm.molloy_reed_randomize(gm.erdos_renyi_gnm(20, 30, directed=True, seed=3))


def test_generate_degree_sequence(monkeypatch):
    import scipy.stats
    for dist in ({1: .5, 2: .3, 3: .2}, scipy.stats.binom(10, .3), scipy.stats.expon(scale=3.0)):
        s = gm.generate_degree_sequence(100, dist, seed=1)
        assert len(s) == 100 and ops.erdos_gallai(s.tolist()) and gm.is_graphic_erdos_gallai(s)
        assert (s == gm.generate_degree_sequence(100, dist, seed=1)).all()
        assert (s != gm.generate_degree_sequence(100, dist, seed=2)).any()
        g = gm.molloy_reed(s, seed=1)
        assert stored_degrees(g, 100) == [int(x) for x in s]
    monkeypatch.setattr(gm, "MAX_SEQUENCE_TRIES", 8)
    with pytest.raises(RuntimeError, match="no graphic sequence"):
        gm.generate_degree_sequence(3, {5: 1.0}, seed=1)
