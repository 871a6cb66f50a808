"""Node layouts on the device (csrc/pp_graph_layout.hip), held to the fixtures made from networkx (tests/golden/layout_vectors.npz).

The Fruchterman-Reingold map is chaotic, so values are compared over short horizons only: every short-horizon case (1, 2, 3, 5 iterations)
through the public ``layout`` to its stored ``rtol`` (16 x the spread of the reference-side evaluations, floor 2**-48, cap 1e-9; form of
tests/tolerance.py) with the iteration count EQUAL, and every recorded single step of a 50-iteration networkx run from networkx's own state,
temperature and step.  The 50-iteration runs themselves are held to networkx's iteration count and to the invariants of the result.  The
kernel settings (target block, source chunks, lanes per list, heavy minimum, batch), determinism, the adjacency, the cheap layouts, ids and
the tensor form follow, at the smallest shapes that reach them.

Run with ``-s`` to print the rtol every case needs next to its bound; DESIGN.md ("Node layouts") records the largest."""
import pathlib

import numpy as np
import pytest
import torch

import pathpyg_amd as pp
from pathpyg_amd import _dispatch, _hip
from pathpyg_amd._lib import HipError, lib
from pathpyg_amd.visualisations import layout as L
from tolerance import assert_embeddings_close, gradient_rtol_needed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "layout_vectors.npz", allow_pickle=False)
CASES = [str(x) for x in GOLDEN["cases"]]
TRAJECTORIES = [str(x) for x in GOLDEN["trajectories"]]
_graphs: dict = {}


def graph_of(g, device=DEV):
    """The Graph of a fixture graph (its edges are stored sorted by source, as the constructor leaves them) and its weight argument."""
    if (g, device) not in _graphs:
        data = pp.Data(edge_index=torch.from_numpy(GOLDEN[f"graph/{g}/edge_index"].astype(np.int64)).to(device), num_nodes=int(GOLDEN[f"graph/{g}/n"]))
        weights = GOLDEN[f"graph/{g}/weights"]
        if weights.size:
            data.edge_weight = torch.from_numpy(weights).to(device)
        _graphs[(g, device)] = (pp.Graph(data), "edge_weight" if weights.size else None)
    return _graphs[(g, device)]


def arguments(name):
    get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
    k = float(get("k"))
    return dict(graph=str(get("graph")), pos0=get("pos0"), k=None if np.isnan(k) else k, fixed=get("fixed").tolist() if bool(get("has_fixed")) else None,
                threshold=float(get("threshold")), center=get("center"), scale=float(get("scale")))


def effective_k(a, n):
    if a["k"] is not None:
        return a["k"]
    return float(a["pos0"].max()) / np.sqrt(n) if a["fixed"] is not None else float(np.sqrt(1.0 / n))


def fixed_mask(a, n):
    if a["fixed"] is None:
        return None
    mask = torch.zeros(n, dtype=torch.bool)
    mask[a["fixed"]] = True
    return mask


def close(got, want, rtol, what):
    want = torch.from_numpy(np.asarray(want))
    print(f"[layout] {what}: needs rtol {gradient_rtol_needed(got, want):.2e} (bound {rtol:.2e})")
    assert_embeddings_close(got, want, rtol=rtol, what=what)


def run_of(name, iterations):
    runs = GOLDEN[f"{name}/runs"]
    return next(r for r in range(len(runs)) if int(runs[r, 0]) == iterations)


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("name", CASES)
def test_short_horizons_match_networkx(name):
    a = arguments(name)
    g, weight = graph_of(a["graph"])
    for r, (iterations, scaled) in enumerate(GOLDEN[f"{name}/runs"].tolist()):
        got = L.layout(g, "spring", weight=weight, k=a["k"], pos=a["pos0"], fixed=a["fixed"], iterations=iterations, threshold=a["threshold"],
                       scale=a["scale"] if scaled else None, center=a["center"], return_tensor=True)
        assert L.last_iterations == int(GOLDEN[f"{name}/run{r}/iterations"]), (name, iterations)
        close(got, GOLDEN[f"{name}/run{r}/pos"], float(GOLDEN[f"{name}/run{r}/rtol"]), f"{name} iterations {iterations} scaled {scaled}")


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_single_steps_from_networkx_states(name):
    a = arguments(name)
    g, weight = graph_of(a["graph"])
    adjacency = _dispatch.graph_layout_adjacency(g, weight)
    dt = float(GOLDEN[f"{name}/dt"])
    for s in GOLDEN[f"{name}/steps"].tolist():
        got, ran, err = _dispatch.graph_fr_layout(adjacency, torch.from_numpy(GOLDEN[f"{name}/step{s}/before"]), effective_k(a, g.n),
                                                  float(GOLDEN[f"{name}/step{s}/t"]), dt, 1, -1.0, fixed=fixed_mask(a, g.n))
        assert ran == 1 and got.is_cuda
        close(got, GOLDEN[f"{name}/step{s}/after"], float(GOLDEN[f"{name}/step{s}/rtol"]), f"{name} step {s}")
        ratio = float(GOLDEN[f"{name}/err_over_threshold"][s])
        assert err == pytest.approx(ratio * a["threshold"], rel=1e-9)


@pytest.mark.parametrize("name", TRAJECTORIES)
def test_long_runs_stop_where_networkx_stops(name):
    a = arguments(name)
    g, weight = graph_of(a["graph"])
    got = L.layout(g, "spring", weight=weight, k=a["k"], pos=a["pos0"], fixed=a["fixed"], iterations=int(GOLDEN[f"{name}/max_iterations"]),
                   threshold=a["threshold"], return_tensor=True)
    assert L.last_iterations == int(GOLDEN[f"{name}/iterations"])
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (g.n, 2)
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    if a["fixed"] is None:                                          # rescaled: mean at the center (0, 0), largest |coordinate| = scale = 1
        assert float(got.mean(0).abs().max()) <= 1e-12
        assert abs(float(got.abs().max()) - 1.0) <= 1e-12
    else:
        start = torch.from_numpy(a["pos0"])
        assert torch.equal(got[a["fixed"]], start[a["fixed"]])
        free = [i for i in range(g.n) if i not in a["fixed"]]
        assert not torch.equal(got[free], start[free])


# ------------------------------------------------------------------ kernel settings
SETTINGS = [dict(block=64), dict(block=128), dict(chunks=1), dict(chunks=2), dict(chunks=3), dict(chunks=7, block=64), dict(group=1), dict(group=8),
            dict(group=64), dict(heavy_min=128), dict(heavy_min=2, group=2), dict(batch=1), dict(batch=7), dict(batch=100)]


def dispatched(name, iterations, **settings):
    a = arguments(name)
    g, weight = graph_of(a["graph"])
    return _dispatch.graph_fr_layout(_dispatch.graph_layout_adjacency(g, weight), torch.from_numpy(a["pos0"]), effective_k(a, g.n), None, None,
                                     iterations, a["threshold"], fixed=fixed_mask(a, g.n), with_stats=True, **settings)


@pytest.mark.parametrize("name", ["random_257", "star_300", "random_1100", "fixed_80"])
def test_every_kernel_setting_agrees_with_the_default(name):
    rtol = float(GOLDEN[f"{name}/run{run_of(name, 3)}/rtol"])
    base, ran, err, stats = dispatched(name, 3)
    assert ran == 3 and stats.target_blocks == -(-base.size(0) // 256) and stats.heavy_grid == 0
    if name == "random_1100":
        assert stats.chunks > 1                                     # (several source tiles: the default splits the source range)
    for settings in SETTINGS:
        got, ran_s, err_s, stats_s = dispatched(name, 3, **settings)
        assert ran_s == 3
        close(got, base.cpu().numpy(), rtol, f"{name} {settings}")
        if "batch" in settings:                                     # the batch never changes a bit
            assert torch.equal(got, base) and err_s == err
        if "chunks" in settings:
            assert stats_s.chunks == settings["chunks"]
        if "block" in settings:
            assert stats_s.target_blocks == -(-base.size(0) // settings["block"])
        if "heavy_min" in settings and name == "star_300":
            assert stats_s.heavy_grid == 1 if settings["heavy_min"] == 128 else stats_s.heavy_grid > 1      # the hub alone / every node with 2 neighbours
    again = dispatched(name, 3)[0]
    assert torch.equal(again, base)                                 # same setting: same bits
    odd = dict(block=64, chunks=5, group=2, heavy_min=16)
    assert torch.equal(dispatched(name, 3, **odd)[0], dispatched(name, 3, **odd)[0])


def test_batches_stop_at_the_converged_iterate():
    """stop_early_100 stops after its 2nd iteration: whatever the batch, later iterates are not applied."""
    want = GOLDEN["stop_early_100/run0/pos"]
    rtol = float(GOLDEN["stop_early_100/run0/rtol"])
    for batch in (0, 1, 2, 3, 50):
        got, ran, err, _ = dispatched("stop_early_100", 5, batch=batch)
        assert ran == 2 and err < arguments("stop_early_100")["threshold"]
        close(got, want, rtol, f"stop_early_100 batch {batch}")


def test_sizes_beyond_int32_are_refused_before_any_launch():
    status = lib().pp_graph_layout_iterate(None, None, None, 2**31 - 1, 0, None, None, 1.0, 0.1, 0.01, 0, 1, 1e-4, 0, 0, 0, 0, 0, None, None, None,
                                          None, 0, None)
    assert status != 0 and "2^31" in lib().pp_last_error().decode()
    status = lib().pp_graph_layout_adj_count(None, 2**30, 5, None, None, 0, None)
    assert status != 0 and "2^31" in lib().pp_last_error().decode()
    with pytest.raises((ValueError, HipError)):
        _hip.graph_layout_iterate(torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), None,
                                  torch.zeros((1, 2), dtype=torch.float64, device=DEV), 1.0, 0.1, 0.01, 1, 1e-4, block=100)


# ------------------------------------------------------------------ adjacency
def dense_of(adjacency, n):
    ptr, nbr, w = (t.cpu() for t in adjacency)
    assert ptr.dtype == torch.int64 and nbr.dtype == torch.int64 and w.dtype == torch.float64 and ptr.numel() == n + 1
    rows = torch.repeat_interleave(torch.arange(n), ptr[1:] - ptr[:-1])
    assert int(ptr[0]) == 0 and int(ptr[-1]) == nbr.numel() and bool((rows != nbr).all())          # no self-loop
    key = rows * n + nbr
    assert bool((key[1:] > key[:-1]).all())                        # sorted by (row, neighbour), one entry per ordered pair
    A = torch.zeros((n, n), dtype=torch.float64)
    A[rows, nbr] = w
    return A, nbr.numel()


@pytest.mark.parametrize("g", ["multi_6", "loops_30", "signed_50", "random_64", "n2"])
def test_adjacency_is_networkx_adjacency(g):
    """The last stored edge of a pair, in either direction, decides the weight; self-loops are dropped; a zero weight stays an entry."""
    graph, weight = graph_of(g)
    want = torch.from_numpy(GOLDEN[f"graph/{g}/A"]).clone()
    loops = int((want.diagonal() != 0).sum())
    want.fill_diagonal_(0.0)
    A, nnz = dense_of(_dispatch.graph_layout_adjacency(graph, weight), graph.n)
    assert torch.equal(A, want)
    ei = graph.data.edge_index.cpu()
    pairs = {(min(u, v), max(u, v)) for u, v in ei.T.tolist() if u != v}
    assert nnz == 2 * len(pairs)
    if g == "multi_6":
        assert loops == 2 and float(A[0, 1]) == 2.0 and float(A[1, 2]) == 4.0 and float(A[3, 4]) == 2.5      # (1,0), (2,1), (4,3): stored last
    # a CPU-resident graph is staged; a weight tensor is the same as the attribute's name
    cpu_graph, _ = graph_of(g, "cpu")
    staged = _dispatch.graph_layout_adjacency(cpu_graph, weight)
    assert all(t.is_cuda for t in staged) and torch.equal(dense_of(staged, graph.n)[0], want)
    if weight is not None:
        assert torch.equal(dense_of(_dispatch.graph_layout_adjacency(graph, graph.data[weight]), graph.n)[0], want)


def test_cpu_graph_gives_the_same_layout():
    a = arguments("loops_30")
    results = []
    for device in (DEV, "cpu"):
        g, weight = graph_of("loops_30", device)
        results.append(L.layout(g, "spring", weight=weight, pos=a["pos0"], iterations=5, return_tensor=True))
    assert results[1].is_cuda and torch.equal(results[0], results[1])
    # an iterable becomes torch.tensor(iterable), as in the reference: float32 for Python floats
    weights = GOLDEN["graph/loops_30/weights"].tolist()
    lists = L.layout(graph_of("loops_30")[0], "spring", weight=weights, pos=a["pos0"], iterations=5, return_tensor=True)
    tensor = L.layout(graph_of("loops_30")[0], "spring", weight=torch.tensor(weights), pos=a["pos0"], iterations=5, return_tensor=True)
    assert torch.equal(lists, tensor) and not torch.equal(lists, results[0])


# ------------------------------------------------------------------ random draws
def test_random_layout():
    g, _ = graph_of("random_257")
    for name in ("random", "rand", None):
        a = L.layout(g, name, seed=5, return_tensor=True)
        assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (257, 2)
        assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
        assert torch.equal(a, L.layout(g, "random", seed=5, return_tensor=True))
    b = L.layout(g, "random", seed=6, return_tensor=True)
    assert not torch.equal(a, b)
    assert 0.4 < float(a.mean()) < 0.6 and float(a.min()) < 0.05 and float(a.max()) > 0.95
    c = L.layout(g, "random", seed=5, center=(2.0, -1.0), return_tensor=True)
    assert torch.equal(c, a + torch.tensor([2.0, -1.0], device=DEV))          # (the float32 sum, as networkx rounds rand + center)
    assert float(c[:, 0].min()) >= 2.0 and float(c[:, 0].max()) <= 3.0 and float(c[:, 1].min()) >= -1.0 and float(c[:, 1].max()) <= 0.0
    d = L.layout(g, "random", seed=5)
    assert list(d) == list(range(257)) and d[3].dtype == np.float32 and np.array_equal(d[3], a[3].cpu().numpy())
    torch.manual_seed(3)
    e = L.layout(g, "random", return_tensor=True)
    torch.manual_seed(3)
    assert torch.equal(e, L.layout(g, "random", return_tensor=True))


def test_spring_draws_are_deterministic_per_seed():
    g, _ = graph_of("random_65")
    a = L.layout(g, "spring", seed=9, iterations=5, return_tensor=True)
    assert torch.equal(a, L.layout(g, "fr", seed=9, iterations=5, return_tensor=True))
    assert not torch.equal(a, L.layout(g, "spring", seed=10, iterations=5, return_tensor=True))
    # a partial dict: the given nodes start where they are told, the others are drawn in [0, dom_size) + center
    start = _dispatch.layout_start(9, 65, 40.0, (100.0, 200.0), torch.full((65, 2), 7.0, dtype=torch.float64), torch.arange(65) < 3, device=DEV)
    assert bool((start[:3] == 7.0).all()) and float(start[3:, 0].min()) >= 100.0 and float(start[3:, 0].max()) < 140.0
    assert float(start[3:, 1].min()) >= 200.0 and float(start[3:, 1].max()) < 240.0
    partial = {0: (0.0, 40.0), 1: (5.0, 5.0)}
    b = L.layout(g, "spring", pos=partial, fixed=[0, 1], seed=9, iterations=5, return_tensor=True)
    assert torch.equal(b, L.layout(g, "spring", pos=partial, fixed=[0, 1], seed=9, iterations=5, return_tensor=True))
    assert b[:2].cpu().tolist() == [[0.0, 40.0], [5.0, 5.0]]


# ------------------------------------------------------------------ the cheap layouts, ids, forms
@pytest.mark.parametrize("n", [1, 2, 7])
def test_circular(n):
    g = pp.Graph(pp.Data(edge_index=torch.zeros((2, 0), dtype=torch.int64, device=DEV), num_nodes=n))
    scale, center = float(GOLDEN["circular_scale"]), GOLDEN["circular_center"]
    for name in ("circular", "circle", "ring", "1d-lattice", "lattice-1d"):
        got = L.layout(g, name, scale=scale, center=center)
        assert list(got) == list(range(n))
        np.testing.assert_allclose(np.array([got[v] for v in range(n)]), GOLDEN[f"circular/{n}"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("n", [1, 5, 16])
def test_grid(n):
    g = pp.Graph(pp.Data(edge_index=torch.zeros((2, 0), dtype=torch.int64, device=DEV), num_nodes=n))
    for name in ("grid", "2d-lattice", "lattice-2d"):
        got = L.layout(g, name)
        np.testing.assert_allclose(np.array([got[v] for v in range(n)]), GOLDEN[f"grid/{n}"], rtol=0, atol=1e-6)
    assert L.Layout(list(range(n)), None, "grid").grid().keys() == got.keys()


def test_keys_are_node_ids_in_index_order():
    ids = ["d", "a", "c", "b"]
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    g = pp.Graph(pp.Data(edge_index=ei, num_nodes=4), mapping=pp.IndexMap(ids))
    got = pp.layout(g, "spring", seed=1)
    assert list(got) == ids and all(isinstance(v, np.ndarray) and v.shape == (2,) and v.dtype == np.float64 for v in got.values())
    tensor = pp.layout(g, "spring", seed=1, return_tensor=True)
    assert tensor.is_cuda and tensor.device == torch.device(DEV) and np.array_equal(np.stack(list(got.values())), tensor.cpu().numpy())
    # dict positions are keyed by id
    placed = pp.layout(g, "spring", pos={"a": (1.0, 2.0), "d": (0.0, 0.0), "zzz": (3.0, 3.0)}, fixed=["a"], seed=1)
    assert placed["a"].tolist() == [1.0, 2.0]
    # a higher-order layer: the ids are tuples
    data = pp.Data(edge_index=torch.tensor([[0, 1], [1, 2]], device=DEV), num_nodes=3, node_sequence=torch.tensor([[0, 1], [1, 2], [2, 3]], device=DEV))
    ho = pp.Graph(data, mapping=pp.IndexMap(ids))
    got = pp.layout(ho, "spring", seed=2)
    assert list(got) == [("d", "a"), ("a", "c"), ("c", "b")]
    assert list(pp.layout(ho, "circular")) == list(got)


def test_public_names():
    assert pp.layout is pp.visualisations.layout.layout and pp.visualisations.Layout is L.Layout
    g, _ = graph_of("n2")
    via_class = L.Layout(g.nodes, g.data.edge_index, "Spring", seed=4, return_tensor=True).generate_layout()
    assert torch.equal(via_class, pp.layout(g, "SPRING", seed=4, return_tensor=True))
    assert torch.equal(via_class, L.Layout(g.nodes, g.data.edge_index, "fr", seed=4, return_tensor=True).generate_nx_layout())
