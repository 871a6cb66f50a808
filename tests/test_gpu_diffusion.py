"""RandomWalk.evolve / stationary_distribution / first_order and the layer methods of MultiOrderModel on the device
(csrc/pp_graph_diffusion.hip), at the smallest shapes that reach each path: every row length and both row kernels, dangling nodes, zero
weights, several workgroups; distributions against the dense matrix power and the exactly rounded yardstick of tests/cpu_ops_diffusion.py
(tolerance: 16 x what the numpy restatement needs against that yardstick, floor 2**-48); stationary distributions against numpy's
eigenvector; a hand-built second-order layer against its first-order chain; the sampler against the propagator; and the header's
properties (a) to (d) as bit-equality.  Run with ``-s`` to print what each comparison needs next to its bound."""
import math
import pathlib

import numpy as np
import pytest
import torch

import cpu_ops_diffusion as ops
import pathpyg_amd as pp
from pathpyg_amd import _dispatch, _hip
from pathpyg_amd.algorithms import centrality, ranking

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOOR = 2.0 ** -48
GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "pagerank_vectors.npz", allow_pickle=False)


def graph_of(ei, n, weights=None, device=DEV, **attrs):
    data = pp.Data(edge_index=torch.as_tensor(np.ascontiguousarray(ei), dtype=torch.int64).reshape(2, -1).to(device), num_nodes=n, **attrs)
    if weights is not None:
        data.edge_weight = torch.as_tensor(np.asarray(weights), dtype=torch.float64).to(device)
    return pp.Graph(data)


class Case:
    """A graph, its RandomWalk and its host structure (the merged entries as RandomWalk weighs them)."""

    def __init__(self, ei, n, weights=None):
        self.ei, self.n, self.weights = np.asarray(ei, dtype=np.int64).reshape(2, -1), n, weights
        self.graph = graph_of(self.ei, n, weights)
        self.rw = pp.processes.RandomWalk(self.graph, weight=None if weights is None else "edge_weight")
        self.src, self.dst, self.w = ops.merged(self.ei, n, weights, count_stored=True)
        self.T, self.prob, self.dangling = ops.table(self.src, self.dst, self.w, n)

    def matrix(self, lazy=0.0):
        return ops.dense_matrix(self.src, self.dst, self.prob, self.dangling, self.n, lazy)

    def in_degrees(self):
        return np.bincount(self.dst, minlength=self.n)


def rows_case():
    """n = 60: pull lists of length 0 (nodes 0, 1), 1 (node 2) and a spread up to the teens, two sinks (6, 7), a node whose only out-entries
    weigh 0 (5: dangling with a non-empty row), a few more zero weights."""
    rng = np.random.default_rng(21)
    n = 60
    ei = rng.integers(0, n, (2, 420))
    ei = ei[:, (ei[1] > 2) & (ei[0] != 6) & (ei[0] != 7)]
    ei = np.concatenate([ei, np.array([[3], [2]]), np.array([[5, 5], [10, 11]])], axis=1)
    w = rng.uniform(0.5, 1.5, ei.shape[1])
    w[ei[0] == 5] = 0.0
    w[::17] = 0.0
    return Case(ei, n, w)


def golden_case(name, weighted=False):
    ei, n = GOLDEN[f"graph/{name}/edge_index"].astype(np.int64), int(GOLDEN[f"graph/{name}/n"])
    return Case(ei, n, np.random.default_rng(5).uniform(0.5, 1.5, ei.shape[1]) if weighted else None)


_cache: dict = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def needed(got, want):
    return ops.rtol_needed(np.asarray(got), np.asarray(want))


def check_trajectory(c, starts, steps, lazy=0.0, heavy_min=0, what=""):
    """evolve(one-hot starts) with keep_all against the exactly rounded yardstick; the bound is 16 x what the numpy restatement needs."""
    ev = c.rw.evolve(torch.tensor(starts), steps, lazy=lazy, keep_all=True, heavy_min=heavy_min)
    got = ev.trajectory.cpu().numpy()
    assert got.shape == (steps + 1, c.n, len(starts)) and torch.equal(ev.final, ev.trajectory[-1])
    for col, s in enumerate(starts):
        x0 = np.zeros(c.n)
        x0[s] = 1.0
        exact = ops.evolve_exact(x0, c.src, c.dst, c.prob, c.dangling, c.n, steps, lazy)
        restated = ops.evolve_bincount(x0, c.src, c.dst, c.prob, c.dangling, c.n, steps, lazy)
        bound = max(FLOOR, 16 * needed(restated, exact))
        need = needed(got[:, :, col], exact)
        print(f"[diffusion] {what} start {s}: needs rtol {need:.2e} (bound {bound:.2e})")
        assert need <= bound, (what, s, need, bound)
        assert np.all(np.abs(got[:, :, col].sum(axis=1) - 1.0) <= c.n * 2.0 ** -52)
    return ev


# ------------------------------------------------------------------ 1. row lengths, both row kernels, dangling nodes, zero weights
@pytest.mark.parametrize("heavy_min", [0, 4])
@pytest.mark.parametrize("lazy", [0.0, 0.25])
def test_row_lengths(heavy_min, lazy):
    c = cached("rows", rows_case)
    deg = c.in_degrees()
    assert deg[0] == 0 and deg[1] == 0 and deg[2] == 1 and {2, 3, 4, 5}.issubset(set(deg.tolist())) and deg.max() >= 9      # light and heavy at heavy_min = 4
    assert c.dangling[[5, 6, 7]].all() and 0 < c.dangling.sum() < c.n and (c.prob == 0).sum() > 2
    check_trajectory(c, [3, 5, 6, 12, 40], 6, lazy, heavy_min, f"rows heavy_min={heavy_min} lazy={lazy}")


def test_hub_row_at_the_default():
    """in_hub: a pull list of 5000 entries, above the default heavy_min (20 chunks of 256, the last one short); several workgroups."""
    c = cached("in_hub", lambda: golden_case("in_hub", weighted=True))
    assert c.in_degrees().max() == 5000 >= _hip.diffusion_heavy_min()
    check_trajectory(c, [0, 1, 2500], 4, 0.0, 0, "in_hub")
    check_trajectory(c, [1, 4999], 3, 0.5, 1, "in_hub heavy_min=1")       # every row that has an entry through the heavy kernel


def test_several_workgroups():
    c = cached("random_3000", lambda: golden_case("random_3000"))
    assert c.n == 3000
    check_trajectory(c, [0, 1500, 2999], 3, 0.0, 0, "random_3000")


def test_dangling_none_some_all():
    ring = Case(np.array([[0, 1, 2, 3], [1, 2, 3, 0]]), 4)
    assert not ring.dangling.any()
    assert ring.rw.evolve(torch.tensor([0]), 6).final.reshape(-1).tolist() == [0.0, 0.0, 1.0, 0.0]
    path = Case(np.array([[0, 1], [1, 2]]), 3)
    ev = path.rw.evolve(torch.tensor([0, 1, 2]), 5, keep_all=True)
    assert ev.final.tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]           # everything ends in the sink, and stays
    assert ev.trajectory[1].tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 1.0]]
    isolated = Case(np.zeros((2, 0), dtype=np.int64), 3)
    assert isolated.dangling.all()
    x = torch.tensor([0.5, 0.25, 0.25], dtype=torch.float64)
    assert isolated.rw.evolve(x, 3).final.tolist() == x.tolist()
    with pytest.raises(ValueError, match="nowhere to start"):
        isolated.rw.evolve("weighted", 1)
    with pytest.raises(ValueError, match="nowhere to start"):
        isolated.rw.evolve("uniform", 1)
    zero = Case(np.array([[0, 1, 1], [1, 0, 2]]), 3, np.array([0.0, 1.0, 3.0]))              # node 0's only entry weighs 0: it is dangling
    assert zero.dangling.tolist() == [True, False, True]
    assert zero.rw.evolve(torch.tensor([1]), 1).final.reshape(-1).tolist() == [0.25, 0.0, 0.75]
    assert zero.rw.evolve(torch.tensor([0]), 4).final.reshape(-1).tolist() == [1.0, 0.0, 0.0]


def test_bad_weights_are_refused():
    for bad in (-1.0, float("nan"), float("inf")):
        g = graph_of(np.array([[0, 1], [1, 0]]), 2, np.array([1.0, bad]))
        with pytest.raises(ValueError, match="finite and not negative"):
            pp.processes.RandomWalk(g, weight="edge_weight").evolve("uniform", 1)


# ------------------------------------------------------------------ 2. evolve
def small_case(n):
    """A weighted graph with two sinks and some zero weights (the sampler test's graph)."""
    rng = np.random.default_rng(n)
    ei = rng.integers(0, n, (2, 6 * n))
    ei = ei[:, (ei[0] != 0) & (ei[0] != n - 1)]                        # nodes 0 and n - 1 are sinks
    w = rng.uniform(0.5, 1.5, ei.shape[1])
    w[::11] = 0.0
    return Case(ei, n, w)


@pytest.mark.parametrize("n", [40, 200])
def test_matrix_power(n):
    c = cached(("small", n), lambda: small_case(n))
    starts, t = [1, 2, n // 2, n - 2], 7
    ev = c.rw.evolve(torch.tensor(starts), t)
    got = ev.final.cpu().numpy()
    want = np.linalg.matrix_power(c.matrix(), t)[starts, :].T                                 # [n, B]
    for col, s in enumerate(starts):
        x0 = np.zeros(n)
        x0[s] = 1.0
        exact = ops.evolve_exact(x0, c.src, c.dst, c.prob, c.dangling, n, t)[-1]
        bound = max(FLOOR, 16 * needed(want[:, col], exact))
        print(f"[diffusion] matrix power n={n} start {s}: needs rtol {needed(got[:, col], want[:, col]):.2e} (bound {bound:.2e})")
        assert needed(got[:, col], want[:, col]) <= bound
    ids = c.rw.evolve(starts, t)                                                              # a list: node ids, which are indices without a mapping
    assert torch.equal(ids.final, ev.final)


@pytest.mark.parametrize("n", [40, 200])
def test_sums_and_tvd(n):
    c = cached(("small", n), lambda: small_case(n))
    rng = np.random.default_rng(1)
    target = rng.uniform(0.0, 1.0, n)
    start = rng.uniform(0.0, 1.0, (n, 3))
    start[:, 1] = 0.0
    start[7, 1] = 5.0
    ev = c.rw.evolve(torch.from_numpy(start), 9, lazy=0.1, target=torch.from_numpy(target), keep_all=True)
    traj = ev.trajectory.cpu().numpy()
    assert traj.shape == (10, n, 3) and tuple(ev.tvd.shape) == (10, 3)
    assert np.all(np.abs(traj.sum(axis=1) - 1.0) <= n * 2.0 ** -52)
    assert np.array_equal(traj[0, :, 1], np.eye(n)[7])                                        # normalised per column
    want = ops.tvd(traj, target / target.sum())
    assert np.all(np.abs(ev.tvd.cpu().numpy() - want) <= n * 2.0 ** -53), np.abs(ev.tvd.cpu().numpy() - want).max()
    one = c.rw.evolve(torch.from_numpy(start[:, 0].copy()), 9, lazy=0.1, target=torch.from_numpy(target))
    assert one.final.dim() == 1 and one.tvd.dim() == 1 and one.trajectory is None            # a 1-D start has no column axis
    assert torch.equal(one.final, ev.final[:, 0]) and torch.equal(one.tvd, ev.tvd[:, 0])
    for name in ("weighted", "uniform"):
        x = c.rw.evolve(name, 0).final.cpu().numpy()
        want0 = c.T / c.T.sum() if name == "weighted" else (c.T > 0) / (c.T > 0).sum()
        assert x.shape == (n,) and needed(x, want0) <= FLOOR


def strongly_connected(n, seed, weighted=True):
    """A ring plus random chords: strongly connected; a self-loop makes it aperiodic."""
    rng = np.random.default_rng(seed)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n])
    ei = np.concatenate([ring, rng.integers(0, n, (2, 3 * n)), np.array([[0], [0]])], axis=1)
    return Case(ei, n, rng.uniform(0.5, 1.5, ei.shape[1]) if weighted else None)


@pytest.mark.parametrize("n,seed", [(30, 1), (120, 2), (300, 3)])
def test_tvd_to_stationary_never_rises(n, seed):
    c = cached(("sc", n, seed), lambda: strongly_connected(n, seed))
    ev = c.rw.evolve(torch.tensor([0, n // 3, n - 1]), 60, target="stationary")
    tvd = ev.tvd.cpu().numpy()
    assert tvd.shape == (61, 3) and tvd[0].min() > 0.5 and tvd[-1].max() < tvd[0].min()
    assert np.all(np.diff(tvd, axis=0) <= 1e-12), np.diff(tvd, axis=0).max()


# ------------------------------------------------------------------ 3. stationary distributions
@pytest.mark.parametrize("n,seed", [(30, 1), (120, 2), (300, 3)])
def test_stationary_against_eigenvector(n, seed):
    c = cached(("sc", n, seed), lambda: strongly_connected(n, seed))
    pi = ops.dominant_left_eigenvector(c.matrix())
    x0 = c.T / c.T.sum()
    for lazy in (0.0, 0.5):
        restated, it = ops.stationary_numpy(x0, c.matrix(lazy), 1e-12, 10000)
        allowed = 4 * np.abs(restated - pi).sum()
        got, iterations = c.rw.stationary_distribution(lazy=lazy, return_iterations=True)
        dist = float(np.abs(got.cpu().numpy() - pi).sum())
        print(f"[diffusion] stationary n={n} lazy={lazy}: L1 {dist:.2e} (allowed {allowed:.2e}), {iterations} iterations (numpy {it})")
        assert got.is_cuda and tuple(got.shape) == (n,) and dist <= allowed
        assert abs(iterations - it) <= 1                                                      # (rounding may move the last step)
    block, its = c.rw.stationary_distribution(lazy=0.5, nstart=torch.tensor([0, 5]), return_iterations=True)
    assert tuple(block.shape) == (n, 2) and len(its) == 2
    for col, s in enumerate((0, 5)):                                                          # unique: the same limit from any start
        restated, it = ops.stationary_numpy(np.eye(n)[s], c.matrix(0.5), 1e-12, 10000)
        assert float(np.abs(block[:, col].cpu().numpy() - pi).sum()) <= 4 * np.abs(restated - pi).sum() and abs(its[col] - it) <= 1


def test_undirected_weighted_gives_strength():
    rng = np.random.default_rng(9)
    n = 50
    pairs = np.array([(u, v) for u in range(n) for v in range(u + 1, n) if rng.random() < 0.2 or v == u + 1]).T
    w = rng.uniform(0.5, 2.0, pairs.shape[1])
    c = Case(np.concatenate([pairs, pairs[::-1]], axis=1), n, np.concatenate([w, w]))
    strength = np.bincount(pairs[0], weights=w, minlength=n) + np.bincount(pairs[1], weights=w, minlength=n)
    got = c.rw.stationary_distribution(lazy=0.5).cpu().numpy()
    assert np.abs(got - strength / strength.sum()).sum() <= 1e-12                             # the start IS the fixed point, up to rounding


def test_bipartite_needs_laziness():
    left, right = 4, 5
    ei = np.array([(u, left + v) for u in range(left) for v in range(right)]).T
    c = Case(np.concatenate([ei, ei[::-1]], axis=1), left + right)
    one_sided = np.zeros(left + right)
    one_sided[:left] = 1.0
    with pytest.raises(centrality.PowerIterationFailedConvergence) as info:
        c.rw.stationary_distribution(nstart=torch.from_numpy(one_sided), max_iter=200)
    assert info.value.max_iter == 200 and info.value.columns is None
    got = c.rw.stationary_distribution(nstart=torch.from_numpy(one_sided), lazy=0.5).cpu().numpy()
    assert np.abs(got - c.T / c.T.sum()).sum() <= 1e-11
    with pytest.raises(centrality.PowerIterationFailedConvergence) as info:                   # a block: the columns that failed are named
        c.rw.stationary_distribution(nstart=torch.from_numpy(np.stack([one_sided, c.T], axis=1)), max_iter=200)
    assert info.value.columns == [0]


# ------------------------------------------------------------------ 4. layers
def hand_layers():
    """Layer 1: a weighted strongly connected graph.  Layer 2 by hand: its nodes are layer 1's entries (a, b), its edges (a, b) -> (b, c) weigh
    w1(a, b) * p1(b -> c), so a walk on it is layer 1's walk seen through a window of two nodes."""
    c1 = strongly_connected(25, 4)
    k = c1.src.size
    index = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(c1.src, c1.dst))}
    e_src, e_dst, e_w = [], [], []
    for (a, b), i in index.items():
        for j in np.flatnonzero(c1.src == b):
            e_src.append(i)
            e_dst.append(int(j))
            e_w.append(c1.w[i] * c1.prob[j])
    seq = torch.tensor(np.stack([c1.src, c1.dst], axis=1), dtype=torch.int64, device=DEV)
    layer2 = graph_of(np.array([e_src, e_dst]), k, np.array(e_w), node_sequence=seq)
    return c1, layer2


def test_second_order_layer_follows_its_first_order_chain():
    c1, layer2 = hand_layers()
    rw2 = pp.processes.RandomWalk(layer2, weight="edge_weight")
    assert rw2.order == 2
    rng = np.random.default_rng(6)
    x1 = rng.uniform(0.0, 1.0, (c1.n, 2))
    x1 /= x1.sum(axis=0)
    x2 = x1[c1.src] * c1.prob[:, None]                                                        # x2(a, b) = x1(a) p1(a -> b)
    t = 5
    ev2 = rw2.evolve(torch.from_numpy(x2), t, keep_all=True)
    ev1 = c1.rw.evolve(torch.from_numpy(x1), t + 1, keep_all=True)
    first = ev2.first_order(trajectory=True).cpu().numpy()
    assert first.shape == (t + 1, c1.n, 2) and torch.equal(ev2.first_order(), ev2.first_order(trajectory=True)[-1])
    want = ev1.trajectory.cpu().numpy()[1:]
    for step in range(t + 1):
        need = needed(first[step], want[step])
        print(f"[diffusion] layer 2 step {step} projected vs layer 1 step {step + 1}: needs rtol {need:.2e} (bound {64 * 2.0 ** -52:.2e})")
        assert need <= 64 * 2.0 ** -52
    assert torch.equal(c1.rw.first_order(ev1.final), ev1.final)                               # order 1: the identity
    vector = rw2.first_order(ev2.final[:, 0].contiguous())
    assert vector.dim() == 1 and torch.equal(vector, ev2.first_order()[:, 0])
    # the projection against numpy, heavy groups included (heavy_min = 2: most first-order nodes end more than one layer node)
    dense = np.zeros((c1.n, 2))
    np.add.at(dense, c1.dst, ev2.final.cpu().numpy())
    for heavy_min in (0, 2):
        assert needed(rw2.first_order(ev2.final, heavy_min=heavy_min).cpu().numpy(), dense) <= FLOOR


def temporal_model():
    events = [(0, 1, 1), (1, 2, 2), (2, 0, 3), (0, 1, 11), (1, 0, 12), (0, 2, 13), (2, 1, 21), (1, 2, 22), (2, 0, 23), (0, 2, 31), (2, 1, 32), (1, 0, 33)]
    ei = torch.tensor([(u, v) for u, v, _ in events], dtype=torch.int64).t().contiguous()
    time = torch.tensor([t for _, _, t in events], dtype=torch.int64)
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=time.to(DEV), num_nodes=3), mapping=pp.IndexMap(["a", "b", "c"]))
    return pp.MultiOrderModel.from_temporal_graph(tg, delta=1, max_order=2)


def test_multi_order_model_methods():
    model = temporal_model()
    second = model.pagerank(2)
    assert list(second) == ["a", "b", "c"] and all(type(v) is float for v in second.values())
    assert abs(sum(second.values()) - 1.0) <= FLOOR                     # (an iteration rounds the mass by about 2**-51, damped by alpha each time)
    tensor = model.pagerank(2, return_tensor=True)
    assert tensor.is_cuda and tensor.tolist() == list(second.values())
    first = model.pagerank(1, alpha=0.7)
    assert first == ranking.pagerank(model.layers[1], 0.7, weight="edge_weight")
    assert model.pagerank(2, 0.5, tol=1e-10) != second
    for order in (1, 2):
        pi = model.stationary_distribution(order, lazy=0.5)
        assert list(pi) == ["a", "b", "c"] and abs(sum(pi.values()) - 1.0) <= 10000 * 2.0 ** -51      # (at most 10000 iterations, 2**-51 each)
    with pytest.raises(ValueError, match="no layer"):
        model.pagerank(3)


# ------------------------------------------------------------------ 5. the sampler against the propagator
@pytest.mark.parametrize("n", [40, 200])
def test_sampler_follows_the_propagator(n):
    """The endpoint frequencies of 20 000 sampled walks at every step (a walk that has ended stays at its last node) lie within
    6 sqrt(p (1 - p) / W) + 1 / W of evolve's distribution."""
    c = cached(("small", n), lambda: small_case(n))
    W, steps = 20000, 8
    nodes = c.rw.run(num_walks=W, steps=steps, start="weighted", seed=1234).nodes.cpu().numpy()
    p = c.rw.evolve("weighted", steps, keep_all=True).trajectory.cpu().numpy()
    at, worst = nodes[:, 0].copy(), 0.0
    for t in range(steps + 1):
        at = np.where(nodes[:, t] >= 0, nodes[:, t], at)
        freq = np.bincount(at, minlength=n) / W
        bound = 6 * np.sqrt(p[t] * (1 - p[t]) / W) + 1 / W
        worst = max(worst, float((np.abs(freq - p[t]) / bound).max()))
        assert np.all(np.abs(freq - p[t]) <= bound), (t, float((np.abs(freq - p[t]) / bound).max()))
    print(f"[diffusion] sampler n={n}: worst deviation {worst:.2f} of the bound")
    assert p[steps][[0, n - 1]].sum() > p[0][[0, n - 1]].sum()                                # the sinks fill up


# ------------------------------------------------------------------ 6. the header's properties (a) to (d), as bit-equality
def run_of(c, block, **kw):
    settings = dict(threshold=-1.0, max_iter=6, lazy=0.1, keep_all=True)
    settings.update(kw)
    return _dispatch.graph_diffusion(c.rw.structure(), c.n, _dispatch.DIFFUSION_WALK, block, settings.pop("threshold"), settings.pop("max_iter"), **settings)


def test_same_bits_every_run_and_under_every_launch_share():
    c = cached("random_3000", lambda: golden_case("random_3000"))
    block = torch.from_numpy(np.random.default_rng(2).uniform(0.0, 1.0, (c.n, 5)))
    target = torch.full((c.n,), 1.0 / c.n, dtype=torch.float64)
    first = run_of(c, block, target=target, want_tvd=True)
    again = run_of(c, block, target=target, want_tvd=True)
    assert torch.equal(first.trajectory, again.trajectory) and torch.equal(first.tvd, again.tvd)
    assert first.grids[0] == math.ceil(c.n / 256)
    with _hip.launch_share(1):                                          # 8 workgroups stride over the 12 ranges
        shared = run_of(c, block, target=target, want_tvd=True)
    assert shared.grids[0] == 8 and torch.equal(first.trajectory, shared.trajectory) and torch.equal(first.tvd, shared.tvd)
    a, b = ranking.pagerank(c.graph, return_tensor=True), None
    with _hip.launch_share(1):
        b = ranking.pagerank(c.graph, return_tensor=True)
    assert torch.equal(a, b)


def test_batch_changes_no_bit_and_max_iter_is_exact():
    c = cached(("sc", 120, 2), lambda: strongly_connected(120, 2))
    block = torch.eye(c.n, dtype=torch.float64)[:, [0, 60]].contiguous()
    want = run_of(c, block, max_iter=7)
    for batch in (1, 4, 16):
        got = run_of(c, block, max_iter=7, batch=batch)
        assert got.iterations == [7, 7] and got.converged == [False, False]
        assert torch.equal(got.trajectory, want.trajectory), batch
    # until a threshold: the same iterate and count whatever the batch; a max_iter that is no multiple of the batch is honoured exactly
    free = run_of(c, block, threshold=1e-9, max_iter=10000, lazy=0.5, keep_all=False)
    assert all(free.converged) and min(free.iterations) > 7
    for batch in (1, 4, 16):
        got = run_of(c, block, threshold=1e-9, max_iter=10000, lazy=0.5, keep_all=False, batch=batch)
        assert got.iterations == free.iterations and torch.equal(got.final, free.final), batch
        cut = run_of(c, block, threshold=1e-9, max_iter=7, lazy=0.5, keep_all=False, batch=batch)
        assert cut.iterations == [7, 7] and cut.converged == [False, False]
        assert torch.equal(cut.final, run_of(c, block, max_iter=7, lazy=0.5).trajectory[7]), batch
    exact = run_of(c, block, threshold=1e-9, max_iter=max(free.iterations), lazy=0.5, keep_all=False, batch=4)
    assert exact.converged == [True, True] and torch.equal(exact.final, free.final)
    short = run_of(c, block, threshold=1e-9, max_iter=max(free.iterations) - 1, lazy=0.5, keep_all=False, batch=4)
    assert short.converged.count(False) >= 1


def test_a_column_does_not_depend_on_its_block():
    """B = 65 (two tiles) against its columns one by one, on the graph with the heavy row: padded widths 1, 64 and 1 again; and a column that
    stopped early keeps the bits of its single run."""
    c = cached("in_hub", lambda: golden_case("in_hub", weighted=True))
    rng = np.random.default_rng(4)
    block = torch.from_numpy(rng.uniform(0.0, 1.0, (c.n, 65)))
    block[:, 3] = 0.0
    block[0, 3] = 1.0
    ev = c.rw.evolve(block, 4, lazy=0.2, target=torch.full((c.n,), 1.0), keep_all=True)
    assert tuple(ev.trajectory.shape) == (5, c.n, 65) and tuple(ev.tvd.shape) == (5, 65)
    for col in (0, 3, 31, 63, 64):
        one = c.rw.evolve(block[:, col].contiguous(), 4, lazy=0.2, target=torch.full((c.n,), 1.0), keep_all=True)
        assert torch.equal(one.trajectory, ev.trajectory[:, :, col]) and torch.equal(one.tvd, ev.tvd[:, col]), col
    narrow = c.rw.evolve(block[:, :3].contiguous(), 4, lazy=0.2)
    assert torch.equal(narrow.final, ev.final[:, :3])
    starts = np.zeros((c.n, 5))                                         # three nodes, the weighted start, the uniform one
    starts[[0, 17, 2500], [0, 1, 2]] = 1.0
    starts[:, 3] = c.T
    starts[:, 4] = 1.0
    many, its = c.rw.stationary_distribution(lazy=0.5, tol=1e-10, nstart=torch.from_numpy(starts), return_iterations=True)
    assert len(set(its)) > 1, its                                       # the premise: the columns stop at different iterations
    for col in range(5):
        single, it = c.rw.stationary_distribution(lazy=0.5, tol=1e-10, nstart=torch.from_numpy(starts[:, col].copy()), return_iterations=True)
        assert it == its[col] and torch.equal(single, many[:, col]), col
