"""pathpyg_amd.processes.RandomWalk on the GPU against the plain restatement of its contract (tests/cpu_ops_walks.py): ``batch.nodes``,
``batch.lengths`` and every PathData tensor must be EQUAL.  Weights are integers or multiples of 2^-10, whose partial sums are exact, so
the float64 running sums carry no rounding a restatement could disagree about; the shapes are the smallest at which each mechanism can go
wrong (bisection ends, start-table block ends, waves and grid ends, every way a walk can end)."""
import numpy as np
import pytest
import torch

import cpu_ops_walks as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def make_graph(pp, edges, n, weight=None, mapping=None):
    ei = torch.tensor(edges, dtype=torch.int64).reshape(-1, 2).t().contiguous().to(DEV)
    data = pp.Data(edge_index=ei, num_nodes=n)
    if weight is not None:
        data.edge_weight = torch.as_tensor(weight).to(DEV)
    return pp.Graph(data, mapping=mapping)


def host_csr(graph, weight="edge_weight"):
    """The graph as the restatement reads it: its stored (row-sorted) order, the weights as exact float64 values."""
    w = None if weight is None else graph.data[weight].cpu().double().tolist()
    return graph.row_ptr.cpu().tolist(), graph.col.cpu().tolist(), w


def check_batch(batch, want, steps, node_sequence, num_first_order=None):
    """nodes, lengths and the five PathData tensors of ``batch`` equal the restated walks ``want``."""
    nodes, lengths = ops.padded(want, steps)
    assert batch.nodes.dtype == torch.int64 and batch.lengths.dtype == torch.int64
    assert batch.nodes.cpu().tolist() == nodes
    assert batch.lengths.cpu().tolist() == lengths
    fields = ops.path_data_fields(want, node_sequence)
    d = batch.to_path_data().data
    assert d.node_sequence.is_cuda and d.node_sequence.dtype == torch.int64 and tuple(d.node_sequence.shape) == (len(fields["node_sequence"]), 1)
    assert d.node_sequence.cpu().tolist() == fields["node_sequence"]
    assert d.edge_index.dtype == torch.int64 and tuple(d.edge_index.shape) == (2, len(fields["edge_index"][0]))
    assert d.edge_index.cpu().tolist() == fields["edge_index"]
    assert d.dag_num_nodes.dtype == torch.int64 and d.dag_num_nodes.cpu().tolist() == fields["dag_num_nodes"]
    assert d.dag_num_edges.dtype == torch.int64 and d.dag_num_edges.cpu().tolist() == fields["dag_num_edges"]
    assert d.dag_weight.dtype == torch.float32 and d.dag_weight.cpu().tolist() == fields["dag_weight"]
    assert d.num_nodes == len(fields["node_sequence"])
    if num_first_order is not None:
        flat = [x[0] for x in fields["node_sequence"]]
        assert batch.visit_counts().cpu().tolist() == np.bincount(np.asarray(flat, dtype=np.int64), minlength=num_first_order).tolist()


def identity(n):
    return [[v] for v in range(n)]


ROW_LENGTHS = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025]


@pytest.fixture(scope="module")
def rows_case(pp):
    """One node per row length (bisection ends), the first or the last entry of every row with weight 0, and a sink; dyadic weights."""
    rng = np.random.default_rng(11)
    n = len(ROW_LENGTHS) + 1
    edges, weight = [], []
    for v, deg in enumerate(ROW_LENGTHS):
        w = rng.integers(0, 5, size=deg).astype(np.float64) / 1024.0
        if deg > 1:
            w[0 if v % 2 else -1] = 0.0
            w[1 if v % 2 else 0] = 3.0 / 1024.0                 # (no row is all zeros)
        else:
            w[0] = 1.0 / 1024.0
        edges += [(v, int(t)) for t in rng.integers(0, n, size=deg)]
        weight += w.tolist()
    g = make_graph(pp, edges, n, torch.tensor(weight, dtype=torch.float64))
    return g, host_csr(g)


def test_row_lengths_and_zero_ends(pp, rows_case):
    g, (row_ptr, col, w) = rows_case
    rw = pp.processes.RandomWalk(g, weight="edge_weight")
    starts = list(range(g.n)) * 12
    want = ops.walks(row_ptr, col, w, 77, 6, starts)
    check_batch(rw.run(steps=6, start=torch.tensor(starts), seed=77), want, 6, identity(g.n), g.n)
    for walk in want:                                           # the restated walks never take an entry of weight 0
        for a, b in zip(walk, walk[1:]):
            assert any(col[j] == b and w[j] > 0 for j in range(row_ptr[a], row_ptr[a + 1]))
    want = ops.walks(row_ptr, col, w, 5, 33, "weighted", num_walks=65)
    check_batch(rw.run(num_walks=65, steps=33, start="weighted", seed=5), want, 33, identity(g.n), g.n)


def test_float32_and_missing_weights(pp, rows_case):
    g, (row_ptr, col, w) = rows_case
    g32 = make_graph(pp, g.data.edge_index.t().cpu().tolist(), g.n, g.data.edge_weight.float())
    want = ops.walks(row_ptr, col, w, 3, 4, "uniform", num_walks=64)
    check_batch(pp.processes.RandomWalk(g32, weight="edge_weight").run(num_walks=64, steps=4, start="uniform", seed=3), want, 4, identity(g.n))
    want = ops.walks(row_ptr, col, None, 3, 4, "weighted", num_walks=64)
    check_batch(pp.processes.RandomWalk(g).run(num_walks=64, steps=4, seed=3), want, 4, identity(g.n))
    counts = make_graph(pp, g.data.edge_index.t().cpu().tolist(), g.n, (g.data.edge_weight * 1024).long())       # an integer attribute
    want = ops.walks(row_ptr, col, [x * 1024 for x in w], 3, 4, "weighted", num_walks=64)
    check_batch(pp.processes.RandomWalk(counts, weight="edge_weight").run(num_walks=64, steps=4, seed=3), want, 4, identity(g.n))


@pytest.mark.parametrize("steps", [0, 1, 2, 33])
def test_single_node_with_a_loop(pp, steps):
    g = make_graph(pp, [(0, 0)], 1)
    rw = pp.processes.RandomWalk(g)
    for W in (1, 63, 64, 65):
        for how in ("weighted", "uniform"):
            check_batch(rw.run(num_walks=W, steps=steps, start=how, seed=W), [[0] * (steps + 1)] * W, steps, [[0]], 1)


def test_steps_and_walk_counts(pp):
    """steps 0, 1, 2, 33 x W 1, 63, 64, 65, 257 on a small multigraph with parallel edges and a sink."""
    edges = [(0, 1), (0, 1), (0, 2), (1, 0), (2, 0), (2, 0), (2, 3), (1, 1), (4, 0)]
    w = [1.0, 2.0, 1.0, 3.0, 0.5, 0.25, 0.25, 1.0, 2.0]
    g = make_graph(pp, edges, 5, torch.tensor(w, dtype=torch.float64))
    row_ptr, col, hw = host_csr(g)
    rw = pp.processes.RandomWalk(g, weight="edge_weight")
    plain = pp.processes.RandomWalk(g)
    for steps in (0, 1, 2, 33):
        for W in (1, 63, 64, 65, 257):
            seed = 1000 * steps + W
            check_batch(rw.run(num_walks=W, steps=steps, seed=seed), ops.walks(row_ptr, col, hw, seed, steps, "weighted", W), steps, identity(5), 5)
    check_batch(plain.run(num_walks=257, steps=5, start="uniform", seed=8), ops.walks(row_ptr, col, None, 8, 5, "uniform", 257), 5, identity(5), 5)


def test_many_walks_per_lane(pp):
    """W = 5000 on 1/1000 of the grid: several walks per lane, the same bits as at full share and as the restatement."""
    from pathpyg_amd import _hip
    rng = np.random.default_rng(2)
    n = 40
    edges = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(200, 2))]
    g = make_graph(pp, edges, n, torch.tensor(rng.integers(0, 4, size=200), dtype=torch.float32))
    row_ptr, col, w = host_csr(g)
    rw = pp.processes.RandomWalk(g, weight="edge_weight")
    full = rw.run(num_walks=5000, steps=3, seed=-7)
    with _hip.launch_share(1):
        small = rw.run(num_walks=5000, steps=3, seed=-7)
        assert _hip.last_persistent_grid() * 256 < 5000
        small_paths = small.to_path_data()
    assert torch.equal(full.nodes, small.nodes) and torch.equal(full.lengths, small.lengths)
    for key in ("node_sequence", "edge_index", "dag_num_nodes", "dag_num_edges", "dag_weight"):
        assert torch.equal(full.to_path_data().data[key], small_paths.data[key])
    check_batch(small, ops.walks(row_ptr, col, w, -7, 3, "weighted", 5000), 3, identity(n), n)


def test_every_way_to_end(pp):
    """Walks that end at step 0 (explicit start on a sink), in the middle and never, in one batch; then a batch where all end at step 0."""
    edges = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 4), (6, 6)]   # 3 and 7 are sinks; 4 <-> 5 and 6 go on for ever
    g = make_graph(pp, edges, 8)
    rw = pp.processes.RandomWalk(g)
    starts = [3, 0, 4, 7, 1, 6, 2, 5, 3] * 15
    want = ops.walks(*host_csr(g, None), 1, 7, starts)
    assert {len(x) - 1 for x in want} == {0, 1, 2, 3, 7}
    check_batch(rw.run(steps=7, start=torch.tensor(starts, device=DEV), seed=1), want, 7, identity(8), 8)
    check_batch(rw.run(steps=7, start=starts, seed=1), want, 7, identity(8), 8)     # (no ids: a list holds indices)
    batch = rw.run(steps=4, start=torch.tensor([3, 7, 7, 3]), seed=1)
    check_batch(batch, [[3], [7], [7], [3]], 4, identity(8), 8)
    empty = batch.to_path_data()
    assert empty.num_paths == 0 and tuple(empty.data.node_sequence.shape) == (0, 1) and tuple(empty.data.edge_index.shape) == (2, 0)
    check_batch(rw.run(steps=0, start=torch.tensor([0, 4]), seed=1), [[0], [4]], 0, identity(8), 8)
    assert rw.run(num_walks=0, steps=3, seed=1).nodes.shape == (0, 4)


def test_graph_of_sinks(pp):
    g = make_graph(pp, [], 5)
    rw = pp.processes.RandomWalk(g)
    check_batch(rw.run(steps=3, start=torch.tensor([0, 4, 2])), [[0], [4], [2]], 3, identity(5), 5)
    for how in ("weighted", "uniform"):
        with pytest.raises(ValueError):
            rw.run(num_walks=3, steps=3, start=how)
    zero = make_graph(pp, [(0, 1), (1, 0)], 2, torch.zeros(2))  # edges, but none of positive weight
    for how in ("weighted", "uniform"):
        with pytest.raises(ValueError):
            pp.processes.RandomWalk(zero, weight="edge_weight").run(num_walks=3, steps=3, start=how)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 3000])
def test_start_tables(pp, n):
    """A ring whose node weights are 0 .. 3 (0: never drawn), with the block ends of the start table inside, at and beyond n."""
    rng = np.random.default_rng(n)
    wt = rng.integers(0, 4, size=n)
    wt[[0, n - 1, min(1023, n - 1)]] = [2, 1, 3]                 # the ends of the table and of its first block can be drawn
    wt[1] = 0
    g = make_graph(pp, [(v, (v + 1) % n) for v in range(n)], n, torch.tensor(wt, dtype=torch.float64))
    row_ptr, col, w = host_csr(g)
    rw = pp.processes.RandomWalk(g, weight="edge_weight")
    for how in ("weighted", "uniform"):
        want = ops.walks(row_ptr, col, w, 21, 2, how, 257)
        batch = rw.run(num_walks=257, steps=2, start=how, seed=21)
        check_batch(batch, want, 2, identity(n))
        assert bool((torch.tensor(wt)[batch.nodes[:, 0].cpu()] > 0).all())


def test_starts_by_id_and_by_index(pp):
    ids = [f"n{v}" for v in range(6)]
    g = make_graph(pp, [(v, (v + 1) % 6) for v in range(6)] + [(0, 3)], 6, mapping=pp.IndexMap(ids))
    rw = pp.processes.RandomWalk(g)
    by_id = rw.run(steps=5, start=["n3", "n0", "n5"], seed=4)
    by_index = rw.run(steps=5, start=torch.tensor([3, 0, 5]), seed=4)
    assert torch.equal(by_id.nodes, by_index.nodes)
    check_batch(by_id, ops.walks(*host_csr(g, None), 4, 5, [3, 0, 5]), 5, identity(6), 6)
    paths = by_id.to_path_data()
    assert paths.mapping is g.mapping and paths.get_walk(0)[0] == "n3"
    with pytest.raises(ValueError):
        rw.run(steps=5, start=["n3", "n9"])
    with pytest.raises(ValueError):
        rw.run(steps=5, start=torch.tensor([6], device=DEV))


def test_seeds(pp):
    rng = np.random.default_rng(4)
    n = 30
    g = make_graph(pp, [(int(a), int(b)) for a, b in rng.integers(0, n, size=(150, 2))], n)
    row_ptr, col, _ = host_csr(g, None)
    rw = pp.processes.RandomWalk(g)
    seen = []
    for seed in (-1, 0, (1 << 63) + 5):
        a = rw.run(num_walks=130, steps=6, seed=seed)
        assert pp.processes.last_seed == seed
        b = rw.run(num_walks=130, steps=6, seed=seed)
        assert torch.equal(a.nodes, b.nodes) and torch.equal(a.lengths, b.lengths)
        check_batch(a, ops.walks(row_ptr, col, None, seed, 6, "weighted", 130), 6, identity(n), n)
        seen.append(a.nodes)
    assert torch.equal(rw.run(num_walks=130, steps=6, seed=(1 << 63) + 5 - (1 << 64)).nodes, seen[2])          # the same int64 bits
    assert torch.equal(rw.run(num_walks=130, steps=6, seed=(1 << 64) - 1).nodes, seen[0])
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])
    torch.manual_seed(3)
    a = rw.run(num_walks=10, steps=3)
    drawn = pp.processes.last_seed
    torch.manual_seed(3)
    assert torch.equal(rw.run(num_walks=10, steps=3).nodes, a.nodes) and pp.processes.last_seed == drawn
    assert torch.equal(rw.run(num_walks=10, steps=3, seed=drawn).nodes, a.nodes)


# ------------------------------------------------------------------ layers of a multi-order model
NAMES = "abcde"


@pytest.fixture(scope="module")
def model(pp):
    """A stream with second-order memory: ... a -> c -> d and ... b -> c -> e ALWAYS, d and e go back to a or b at random.  Every ground
    walk is a run of consecutive timestamps, runs are far apart, so with delta = 1 the time-respecting paths are the runs' windows."""
    rng = np.random.default_rng(5)
    a, b, c, d, e = range(5)
    events, t = [], 0
    for _ in range(260):
        v = int(rng.integers(0, 5))
        prev = int(rng.choice([a, b]))
        for _ in range(int(rng.integers(3, 7))):
            if v == c:
                nxt = d if prev == a else e
            elif v in (a, b):
                nxt = c
            else:
                nxt = int(rng.choice([a, b]))
            events.append((v, nxt, t))
            prev, v, t = v, nxt, t + 1
        t += 10
    ei = torch.tensor([(u, v) for u, v, _ in events], dtype=torch.int64).t().contiguous()
    time = torch.tensor([x for _, _, x in events], dtype=torch.int64)
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=time.to(DEV), num_nodes=5), mapping=pp.IndexMap(list(NAMES)))
    return pp.MultiOrderModel.from_temporal_graph(tg, delta=1, max_order=3)


def layer_csr(layer):
    return host_csr(layer) + (layer.data.node_sequence.cpu().tolist(),)


@pytest.mark.parametrize("k", [2, 3])
def test_higher_order_layers(pp, model, k):
    layer = model.layers[k]
    row_ptr, col, w, seq = layer_csr(layer)
    rw = pp.processes.RandomWalk(layer, weight="edge_weight", first_order_mapping=model.layers[1].mapping)
    want = ops.walks(row_ptr, col, w, 13, 9, "weighted", 300)
    batch = rw.run(num_walks=300, steps=9, seed=13)
    check_batch(batch, want, 9, seq, 5)
    paths = batch.to_path_data()
    assert paths.mapping is model.layers[1].mapping
    grams = {tuple(seq[u]) + (seq[v][-1],) for u in range(len(seq)) for v in col[row_ptr[u]:row_ptr[u + 1]]}
    nodes, start = paths.data.node_sequence[:, 0].cpu().tolist(), 0
    assert paths.num_paths > 0
    for length in paths.data.dag_num_nodes.cpu().tolist():
        fo = nodes[start:start + length]
        assert length >= k + 1 and all(tuple(fo[i:i + k + 1]) in grams for i in range(length - k))
        start += length
    uniform = rw.run(num_walks=64, steps=3, start="uniform", seed=13)
    check_batch(uniform, ops.walks(row_ptr, col, w, 13, 3, "uniform", 64), 3, seq, 5)
    plain = pp.processes.RandomWalk(layer, weight="edge_weight").run(num_walks=10, steps=2, seed=1).to_path_data()
    assert not plain.mapping.has_ids                            # without a first-order mapping the ids are node_sequence's integers


def restated_paths(pp, model, order, num_walks, steps, seed):
    row_ptr, col, w, seq = layer_csr(model.layers[order])
    walks = [ops.first_order(x, seq) for x in ops.walks(row_ptr, col, w, seed, steps, "weighted", num_walks) if len(x) > 1]
    out = []
    for device in (DEV, None):                                  # device-resident, and host-resident (the generic kernels)
        paths = pp.PathData(model.layers[1].mapping, device=device)
        paths.append_walks([[NAMES[v] for v in x] for x in walks], [1.0] * len(walks))
        out.append(paths)
    return out


@pytest.mark.parametrize("order, expect", [(2, 2), (1, 1)])
def test_sampled_walks_carry_their_order(pp, model, order, expect):
    """from_path_data of the sampled walks has the layers of from_path_data of the restated walks, estimate_order gives the same integer
    on both, and that integer is the order of the layer the walks came from."""
    seed = 31
    sampled = model.sample_walks(order, 4096, 8, seed=seed)
    restated, host = restated_paths(pp, model, order, 4096, 8, seed)
    for key in ("node_sequence", "edge_index", "dag_num_nodes", "dag_num_edges", "dag_weight"):
        assert torch.equal(sampled.data[key], restated.data[key]), key
    assert sampled.mapping is model.layers[1].mapping
    got = pp.MultiOrderModel.from_path_data(sampled, max_order=3)
    want = pp.MultiOrderModel.from_path_data(restated, max_order=3)
    for k in (1, 2, 3):
        for key in ("edge_index", "edge_weight", "node_sequence"):
            assert torch.equal(got.layers[k].data[key], want.layers[k].data[key]), (k, key)
    assert got.estimate_order(sampled) == want.estimate_order(restated) == expect
    assert pp.MultiOrderModel.from_path_data(host, max_order=3).estimate_order(host) == expect


# ------------------------------------------------------------------ refusals and general weights
def test_refusals(pp):
    from pathpyg_amd import _lib
    g = make_graph(pp, [(0, 1), (1, 0)], 2)
    with pytest.raises(_lib.HipError, match="-4"):
        pp.processes.RandomWalk(g).run(num_walks=1 << 20, steps=2047)               # 2^20 * 2048 = 2^31: refused by arithmetic
    layer2 = pp.Graph(pp.Data(edge_index=torch.tensor([[0], [1]], device=DEV), num_nodes=2, node_sequence=torch.tensor([[0, 1], [1, 0]], device=DEV)))
    with pytest.raises(_lib.HipError, match="-4"):
        pp.processes.RandomWalk(layer2).run(num_walks=1 << 20, steps=2046)          # the order counts: 2^20 * (2046 + 2)
    for bad in (-1.0, float("nan"), float("inf")):
        for dtype in (torch.float32, torch.float64):
            h = make_graph(pp, [(0, 1), (1, 0), (1, 1)], 2, torch.tensor([1.0, bad, 1.0], dtype=dtype))
            with pytest.raises(ValueError):
                pp.processes.RandomWalk(h, weight="edge_weight").run(num_walks=4, steps=2)
            with pytest.raises(ValueError):
                pp.processes.RandomWalk(h, weight="edge_weight").table()


def test_general_float32_weights(pp):
    """Random float32 weights: every step is a stored edge of positive weight, and two runs agree bit for bit."""
    rng = np.random.default_rng(9)
    n, m = 300, 4000
    edges = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(m, 2))]
    w = rng.random(m).astype(np.float32)
    w[rng.integers(0, m, size=400)] = 0.0
    g = make_graph(pp, edges, n, torch.tensor(w))
    positive = {(int(a), int(b)) for (a, b), x in zip(g.data.edge_index.t().cpu().tolist(), g.data.edge_weight.cpu().tolist()) if x > 0}
    rw = pp.processes.RandomWalk(g, weight="edge_weight")
    a = rw.run(num_walks=2000, steps=12, seed=6)
    b = pp.processes.RandomWalk(g, weight="edge_weight").run(num_walks=2000, steps=12, seed=6)
    assert torch.equal(a.nodes, b.nodes) and torch.equal(a.lengths, b.lengths)
    nodes, lengths = a.nodes.cpu().tolist(), a.lengths.cpu().tolist()
    assert max(lengths) == 12
    for walk, length in zip(nodes, lengths):
        assert all((walk[t], walk[t + 1]) in positive for t in range(length)) and all(x == -1 for x in walk[length + 1:])
        assert length == 12 or not any(u == walk[length] for u, _ in positive)      # a walk ends only where nothing leads on
    pa, pb = a.to_path_data(), b.to_path_data()
    for key in ("node_sequence", "edge_index", "dag_num_nodes", "dag_num_edges", "dag_weight"):
        assert torch.equal(pa.data[key], pb.data[key])
