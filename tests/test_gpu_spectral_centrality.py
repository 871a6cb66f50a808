"""eigenvector_centrality and katz_centrality on the device (csrc/pp_graph_power.hip) through the public functions, held to the fixtures made
from networkx (tests/golden/spectral_centrality_vectors.npz): values to each case's stored ``rtol`` (16 x what separates networkx from
exactly rounded sums, floor 2**-48; form of tests/tolerance.py), iteration counts EQUAL (every case keeps its error at least 1e-6 relative
away from the threshold), raises where networkx raised.  The kernel paths (lanes per row, the heavy launch, several workgroups), the batch
logic (first converging iterate, max_iter honoured exactly), determinism, ``Graph.simple_predecessors()``, staging, IDs and input forms
follow, at the smallest shapes that reach them.

Measured on an MI355X (2026-10-21): the largest rtol needed over all fixture cases and kernel settings is written next to the largest
allowed one in DESIGN.md; run with ``-s`` to print each."""
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_spectral as ops
import pathpyg_amd as pp
from pathpyg_amd import _dispatch, _hip
from pathpyg_amd.algorithms import centrality
from tolerance import assert_embeddings_close, gradient_rtol_needed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "spectral_centrality_vectors.npz", allow_pickle=False)
NAMES = [str(x) for x in GOLDEN["names"]]
_cases: dict = {}
_graphs: dict = {}


def case(name):
    if name not in _cases:
        get = lambda key: GOLDEN[f"{name}/{key}"]  # noqa: E731
        g = str(get("graph"))
        beta, nstart, weights = get("beta"), get("nstart"), get("weights")
        _cases[name] = dict(
            name=name, edge_index=GOLDEN[f"graph/{g}/edge_index"].astype(np.int64), n=int(GOLDEN[f"graph/{g}/n"]), kind=str(get("kind")),
            max_iter=int(get("max_iter")), tol=float(get("tol")), alpha=float(get("alpha")), beta=float(beta[0]) if beta.size == 1 else beta,
            nstart=nstart if nstart.size else None, normalized=bool(get("normalized")), weights=weights if weights.size else None,
            raised=bool(get("raised")), values=torch.from_numpy(get("values")), iterations=int(get("iterations")), rtol=float(get("rtol")))
    return _cases[name]


def graph_of(ei, n, device=DEV, ids=None, weights=None):
    """A Graph from any edge list (the constructor sorts by source and permutes the attribute alike)."""
    data = pp.Data(edge_index=torch.as_tensor(np.ascontiguousarray(ei), dtype=torch.int64).reshape(2, -1).to(device), num_nodes=n)
    if weights is not None:
        data.edge_weight = torch.as_tensor(np.asarray(weights), dtype=torch.float64).to(device)
    return pp.Graph(data, mapping=None if ids is None else pp.IndexMap(list(ids)))


def case_graph(c, device=DEV):
    key = (c["name"], device)
    if key not in _graphs:
        _graphs[key] = graph_of(c["edge_index"], c["n"], device, weights=c["weights"])
    return _graphs[key]


def public(c, g, **kw):
    weight = "edge_weight" if c["weights"] is not None else None
    if c["kind"] == "eigenvector":
        return centrality.eigenvector_centrality(g, c["max_iter"], c["tol"], c["nstart"], weight, **kw)
    return centrality.katz_centrality(g, c["alpha"], c["beta"], c["max_iter"], c["tol"], c["nstart"], c["normalized"], weight, **kw)


def dispatched(c, g=None, max_iter=None, **kw):
    """``(values, iterations, converged, stats)`` of a fixture case through _dispatch.graph_power_centrality."""
    eig = c["kind"] == "eigenvector"
    beta = c["beta"] if isinstance(c["beta"], float) else torch.from_numpy(c["beta"])
    return _dispatch.graph_power_centrality(
        case_graph(c) if g is None else g, _hip.POWER_EIGENVECTOR if eig else _hip.POWER_KATZ, c["n"] * c["tol"],
        c["max_iter"] if max_iter is None else max_iter, alpha=c["alpha"], beta=beta, start=None if c["nstart"] is None else torch.from_numpy(c["nstart"]),
        normalized=c["normalized"], weight="edge_weight" if c["weights"] is not None else None, with_stats=True, **kw)


def held(c, got, what):
    got = got.cpu() if isinstance(got, torch.Tensor) else torch.tensor(list(got), dtype=torch.float64)
    print(f"[spectral] {what}: needs rtol {gradient_rtol_needed(got, c['values']):.2e} (bound {c['rtol']:.2e})")
    assert_embeddings_close(got, c["values"], rtol=c["rtol"], what=what)


# ------------------------------------------------------------------ 1. fixtures through the public functions
@pytest.mark.parametrize("name", NAMES)
def test_fixture(name):
    c = case(name)
    g = case_graph(c)
    if c["raised"]:
        with pytest.raises(centrality.PowerIterationFailedConvergence) as info:
            public(c, g)
        assert info.value.max_iter == c["max_iter"]
        assert dispatched(c)[1:3] == (c["max_iter"], False)             # the iteration count behind the public call
        return
    got = public(c, g)
    assert dispatched(c)[1:3] == (c["iterations"], True)
    assert list(got) == list(range(c["n"])) and all(type(v) is float for v in got.values())
    held(c, got.values(), name)
    tensor = public(c, g, return_tensor=True)                           # the tensor route: the same values, on the device
    assert tensor.is_cuda and tensor.dtype == torch.float64 and tensor.tolist() == list(got.values())


def test_known_values():
    assert public(case("single_eig"), case_graph(case("single_eig"))) == {0: 1.0}
    assert public(case("single_katz"), case_graph(case("single_katz"))) == {0: 1.0}
    assert public(case("single_loop_eig"), case_graph(case("single_loop_eig"))) == {0: 1.0}
    held(case("isolated3_katz"), public(case("isolated3_katz"), case_graph(case("isolated3_katz"))).values(), "isolated3")


# ------------------------------------------------------------------ 2. kernel paths
def in_degrees(c):
    _, dst, _ = ops.simple_edges(c["edge_index"], c["n"])
    return np.bincount(dst, minlength=c["n"])


@pytest.mark.parametrize("heavy_min", [0, 4])
@pytest.mark.parametrize("group", [1, 8, 64])
@pytest.mark.parametrize("name", ["random_300_eig", "random_300_katz", "in_hub_eig", "in_hub_katz"])
def test_lanes_per_row_and_heavy_launch(name, group, heavy_min):
    c = case(name)
    values, iterations, converged, stats = dispatched(c, group=group, heavy_min=heavy_min)
    assert converged and iterations == c["iterations"]
    held(c, values, f"{name} group {group} heavy_min {heavy_min}")
    deg = in_degrees(c)
    threshold = heavy_min or _hip.power_heavy_min()
    assert (stats.heavy_grid > 0) == bool((deg >= threshold).any())
    if heavy_min == 4:
        assert (deg >= 4).any() and (deg < 4).any() and stats.heavy_grid > 0           # both launches have rows


@pytest.mark.parametrize("name", ["random_3000_eig", "random_3000_katz", "hub_ring_eig", "hub_ring_katz"])
def test_many_workgroups(name):
    c = case(name)
    values, iterations, converged, stats = dispatched(c)
    assert converged and iterations == c["iterations"]
    assert stats.light_grid > 1
    held(c, values, name)


@pytest.mark.parametrize("name", ["random_3000_eig", "hub_ring_katz", "in_hub_eig", "random_300_katz_weighted"])
def test_same_bits_on_every_run(name):
    c = case(name)
    first, second = dispatched(c)[0], dispatched(c)[0]
    assert torch.equal(first, second)
    assert torch.equal(first, public(c, case_graph(c), return_tensor=True))


@pytest.mark.parametrize("batch", [0, 8, 9])
@pytest.mark.parametrize("name", ["random_300_katz", "in_hub_eig", "random_50_eig"])
def test_first_converging_iterate(name, batch):
    c = case(name)
    k = c["iterations"]
    assert k >= 2 and (batch == 0 or k % batch)                         # (8 and 9 divide none of 21, 20 and 12)
    default = dispatched(c)[0]
    values, iterations, converged, _ = dispatched(c, max_iter=k, batch=batch)
    assert converged and iterations == k and torch.equal(values, default)
    values, iterations, converged, _ = dispatched(c, max_iter=k - 1, batch=batch)
    assert not converged and iterations == k - 1 and not torch.equal(values, default)
    values, iterations, converged, _ = dispatched(c, max_iter=10 * k, batch=batch)     # later batches change nothing
    assert converged and iterations == k and torch.equal(values, default)


def test_batch_below_eight_is_refused():
    with pytest.raises(ValueError, match="batch"):
        dispatched(case("k5_eig"), batch=3)


# ------------------------------------------------------------------ 3. Graph.simple_predecessors
def host_transpose(ei, n):
    src, dst, _ = ops.simple_edges(ei, n)
    order = np.lexsort((src, dst))                                      # by column, sources ascending inside
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=ptr[1:])
    return ptr, src[order], order


def test_simple_predecessors():
    multi = np.array([[3, 0, 0, 2, 2, 2, 1, 4, 0, 3], [1, 2, 2, 2, 0, 0, 1, 0, 4, 1]])       # parallel edges, self-loops; node 5 is isolated
    strict = np.array([[0, 0, 1, 2, 3, 3], [1, 3, 1, 0, 0, 2]])                             # its own simple structure
    for ei, n, own in ((multi, 6, False), (strict, 5, True)):
        g = graph_of(ei, n)
        assert (g.simple_successors()[3] is None) == own
        col_ptr, row, perm = g.simple_predecessors()
        want_ptr, want_row, want_perm = host_transpose(ei, n)
        assert col_ptr.is_cuda and col_ptr.dtype == row.dtype == perm.dtype == torch.int64
        assert col_ptr.tolist() == want_ptr.tolist() and row.tolist() == want_row.tolist() and perm.tolist() == want_perm.tolist()
        assert g.simple_predecessors()[0] is col_ptr                     # kept
    empty = graph_of(np.zeros((2, 0)), 3)
    col_ptr, row, perm = empty.simple_predecessors()
    assert col_ptr.tolist() == [0, 0, 0, 0] and row.numel() == perm.numel() == 0


# ------------------------------------------------------------------ 4. parallel edges and weights
def test_parallel_edges_collapse_and_named_weights_sum():
    rng = np.random.default_rng(5)
    n = 40
    ei = rng.integers(0, n, (2, 400))
    ei = np.concatenate([ei, ei[:, :150], ei[:, :40]], axis=1)            # multiplicities 1, 2 and 3 (and what chance adds)
    src, dst, mult = ops.simple_edges(ei, n, np.ones(ei.shape[1]))
    assert mult.max() >= 3 and mult.min() == 1
    multi = graph_of(ei, n, weights=np.ones(ei.shape[1]))
    copy = graph_of(np.stack([src, dst]), n, weights=mult)
    for fn, kw in ((centrality.eigenvector_centrality, {}), (centrality.katz_centrality, dict(alpha=0.02))):
        unit = fn(multi, return_tensor=True, **kw)
        assert torch.equal(unit, fn(copy, return_tensor=True, **kw))     # weight=None: every distinct edge counts 1
        by_mult = fn(multi, weight="edge_weight", return_tensor=True, **kw)
        assert torch.equal(by_mult, fn(copy, weight="edge_weight", return_tensor=True, **kw))
        assert not torch.equal(by_mult, unit)
    want, iterations = ops.katz(ei, n, 0.02, weights=np.ones(ei.shape[1]))
    rtol = ops.derived_rtol(want, ops.katz_exact(ei, n, iterations, 0.02, weights=np.ones(ei.shape[1])))      # the fixtures' rule
    got = centrality.katz_centrality(multi, 0.02, weight="edge_weight", return_tensor=True).cpu()
    print(f"[spectral] katz by multiplicity: needs rtol {gradient_rtol_needed(got, torch.from_numpy(want)):.2e} (bound {rtol:.2e})")
    assert_embeddings_close(got, torch.from_numpy(want), rtol=rtol, what="katz by multiplicity")


# ------------------------------------------------------------------ 5. staging and IDs
def test_cpu_resident_graph_gives_the_same_dict():
    for name in ("random_300_katz_weighted", "random_50_eig", "multi_02_eig"):
        c = case(name)
        assert public(c, case_graph(c, "cpu")) == public(c, case_graph(c))
    c = case("random_50_eig")
    assert public(c, case_graph(c, "cpu"), return_tensor=True).is_cuda     # the compute device


def test_string_ids_in_unsorted_order():
    c = case("multi_03_katz")
    ids = [f"node{(7 * i + 3) % c['n']:02d}" for i in range(c["n"])]        # index i has the ID ids[i]: not sorted
    assert ids != sorted(ids) and len(set(ids)) == c["n"]
    plain = public(c, case_graph(c))
    named = public(c, graph_of(c["edge_index"], c["n"], ids=ids))
    assert list(named) == ids and list(named.values()) == list(plain.values())


def test_second_order_layer_returns_tuple_keys():
    events = [("a", "b", 1), ("b", "c", 5), ("c", "d", 9), ("c", "e", 9), ("c", "f", 11), ("f", "a", 13), ("a", "g", 18), ("b", "f", 21),
              ("a", "g", 26), ("c", "f", 27), ("h", "f", 27), ("g", "h", 28), ("a", "c", 30), ("a", "b", 31), ("c", "h", 32), ("f", "h", 33),
              ("b", "i", 42), ("i", "b", 42), ("c", "i", 47), ("h", "i", 50)]
    t = pp.TemporalGraph.from_edge_list(events, device=DEV)
    layer = pp.MultiOrderModel.from_temporal_graph(t, delta=15, max_order=2).layers[2]
    n, ei = layer.n, layer.data.edge_index.cpu().numpy()
    assert n > 2 and ei.shape[1] > 2
    ids = [layer.mapping.to_id(i) for i in range(n)]
    got = centrality.katz_centrality(layer, alpha=0.05)
    assert list(got) == ids and all(isinstance(i, tuple) and len(i) == 2 for i in got)
    want, iterations = ops.katz(ei, n, 0.05)
    assert _dispatch.graph_power_centrality(layer, _hip.POWER_KATZ, n * 1e-06, 1000, alpha=0.05, beta=1.0)[1:] == (iterations, True)
    rtol = ops.derived_rtol(want, ops.katz_exact(ei, n, iterations, 0.05))                 # the fixtures' rule
    values = torch.tensor(list(got.values()), dtype=torch.float64)
    print(f"[spectral] order-2 layer: needs rtol {gradient_rtol_needed(values, torch.from_numpy(want)):.2e} (bound {rtol:.2e})")
    assert_embeddings_close(values, torch.from_numpy(want), rtol=rtol, what="katz on the order-2 layer")


# ------------------------------------------------------------------ 6. input forms
def test_vector_forms_agree():
    c = case("random_300_katz_beta_vector")
    g = case_graph(c)
    beta = c["beta"]
    start = np.random.default_rng(3).uniform(0.1, 1.0, c["n"])
    forms = lambda v: (torch.from_numpy(v), torch.from_numpy(v).to(DEV), v, v.tolist(), dict(enumerate(v.tolist())),  # noqa: E731
                       dict(reversed(list(enumerate(v.tolist())))))
    want = centrality.katz_centrality(g, 0.05, beta, nstart=start)
    held(c, centrality.katz_centrality(g, 0.05, beta).values(), "beta vector")
    for b, s in zip(forms(beta), forms(start)):
        assert centrality.katz_centrality(g, 0.05, b, nstart=s) == want
    want = centrality.eigenvector_centrality(g, nstart=start)
    for s in forms(start):
        assert centrality.eigenvector_centrality(g, nstart=s) == want
    assert centrality.katz_centrality(g, 0.05, 2) == centrality.katz_centrality(g, 0.05, 2.0) == centrality.katz_centrality(g, 0.05, np.full(c["n"], 2.0))


def test_any_start_vector_ends_by_max_iter():
    c = case("random_50_eig")
    g = case_graph(c)
    start = np.zeros(c["n"])
    start[:2] = (1.0, -1.0)                                             # sums to zero: the first division leaves no finite iterate
    with pytest.raises(centrality.PowerIterationFailedConvergence):
        centrality.eigenvector_centrality(g, max_iter=20, nstart=start)
    values, iterations, converged = _dispatch.graph_power_centrality(g, _hip.POWER_EIGENVECTOR, c["n"] * 1e-06, 20, start=torch.from_numpy(start))
    assert iterations == 20 and not converged and not bool(torch.isfinite(values).any())
    start[:] = np.random.default_rng(4).uniform(-1.0, 1.0, c["n"])
    values, iterations, converged = _dispatch.graph_power_centrality(g, _hip.POWER_KATZ, c["n"] * 1e-06, 30, alpha=0.05, beta=1.0,
                                                                     start=torch.from_numpy(start))
    assert 1 <= iterations <= 30 and (converged or iterations == 30)
    if converged:
        assert torch.equal(centrality.katz_centrality(g, 0.05, nstart=start, max_iter=30, return_tensor=True), values)
    else:
        with pytest.raises(centrality.PowerIterationFailedConvergence):
            centrality.katz_centrality(g, 0.05, nstart=start, max_iter=30)
