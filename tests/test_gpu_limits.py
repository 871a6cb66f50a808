"""GPU tests of the three De Bruijn builders at the limits of fp32 merged weights and int32 counts: the generic kernels (``pp_temporal_*`` /
``pp_linegraph_*`` / ``pp_coalesce_*``), the order-2 builder (``pp_debruijn2_*``, what ``from_temporal_graph(max_order=2)`` runs) and the
level-by-level builder (``pp_multiorder_*``, ``max_order >= 3``).  Every test asserts the route it took, so that a changed threshold cannot
move it off the kernel it pins.

  A  fractional weights on node pairs with hundreds to tens of thousands of events: merged weights are PyG's left-to-right fp32 sums
  B  merged weights past 2^24: unit weights give float32(count) on every route (the reference's sum of ones stops at 2^24), integer
     weights are within 1e-6 of the float64 sum
  C  counts past 2^31: the int64 offsets of the temporal and line-graph lifts, an order-2 edge of more than 2^31 instances, and a refusal
     (never a wrapped count) where a builder's counts end (the C tests allocate up to ~40 GB of device memory each)
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TWO24 = 1 << 24
TWO31 = 1 << 31


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


@pytest.fixture(autouse=True)
def _release_device_memory():
    torch.cuda.reset_peak_memory_stats()
    yield
    gc.collect()
    torch.cuda.empty_cache()
    print(f" [peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB]")


def _level_by_level(model) -> bool:
    return "layers" in getattr(model, "sizes", {})


def _build(pp, g, delta, route, K):
    """``from_temporal_graph`` on one route: "order2" (K = 2, the order-2 builder), "levels" (K >= 3, the level-by-level builder),
    "generic" (the generic kernels, ``FUSED_BUILDER = False``) or "handed_back" (K >= 3: the level-by-level builder refuses the stream)."""
    from pathpyg_amd.core import multi_order_model as mm
    if route == "generic":
        mm.FUSED_BUILDER = False
        try:
            model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=K)
        finally:
            mm.FUSED_BUILDER = True
    else:
        model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=K)
    fused = getattr(model, "_pp_fused", None) is not None
    if route == "order2":
        assert K == 2 and fused, "from_temporal_graph(max_order=2) did not take the order-2 builder"
    elif route == "levels":
        assert K >= 3 and _level_by_level(model), f"from_temporal_graph(max_order={K}) did not take the level-by-level builder"
    else:
        assert not fused and not _level_by_level(model), f"{route}: a fast builder kept the stream"
    return model


def _graph(pp, src, dst, t, n, w=None):
    data = pp.Data(edge_index=torch.from_numpy(np.stack((src, dst))).to(DEV), time=torch.from_numpy(t).to(DEV), num_nodes=n)
    if w is not None:
        data["edge_weight"] = torch.from_numpy(w).to(DEV)
    return pp.TemporalGraph(data)


# ------------------------------------------------------------------ A: fractional weights on long runs, bit for bit against the oracle
CHAINS = (65, 129, 200, 513, 4000)      # a -> b -> c -> d -> e, every hop L times: runs of L instances in layers 1..4
FANS = (300, 3000)                      # L events a -> b inside one window, then one b -> c: one order-2 edge of L instances into one out-event
PAIRS = (65, 129, 513, 5000, 70000)     # x -> y with y a sink: layer-1 runs of L events


def _long_run_stream(seed):
    """Sparse background traffic (300 nodes, 20 000 events, few continuations) and, on nodes of their own, the runs above.  The sizes cross
    the order-2 builder's hub threshold (64 events per node and side), the level-by-level builder's long pairs (kMoLongRun = 128) and wave /
    workgroup type classes (256 children), and the generic coalesce's long runs (kLongRun = 512); every type keeps at most 4096 children,
    so the level-by-level builder keeps the stream.  delta = 10."""
    rng = np.random.default_rng(seed)
    n_bg, m_bg = 300, 20_000
    src, dst, t = [rng.integers(0, n_bg, m_bg)], [rng.integers(0, n_bg, m_bg)], [rng.integers(0, 4_000, m_bg)]
    node = n_bg
    for L in CHAINS:        # hop h of instance i at 40 i + 10 h: every event continued by exactly one event of the next hop
        i = np.arange(L)
        for h in range(4):
            src.append(np.full(L, node + h)); dst.append(np.full(L, node + h + 1)); t.append(40 * i + 10 * h)
        node += 5
    for L in FANS:          # (ties inside the window: the stable time order decides the order of the instances)
        src += [np.full(L, node), np.full(1, node + 1)]; dst += [np.full(L, node + 1), np.full(1, node + 2)]
        t += [rng.integers(100, 110, L), np.full(1, 110)]
        node += 3
    for L in PAIRS:
        src.append(np.full(L, node)); dst.append(np.full(L, node + 1)); t.append(rng.integers(0, 10 * L, L))
        node += 2
    src, dst, t = np.concatenate(src), np.concatenate(dst), np.concatenate(t)
    perm = rng.permutation(src.size)             # (arrival order is not time order: the builders sort, stably)
    w = (rng.random(src.size) + 0.25).astype(np.float32)
    return src[perm], dst[perm], t[perm], w, node, 10


def _oracle(src, dst, t, n, delta, K, w=None):
    from oracle import model as om
    ei, tt = torch.from_numpy(np.stack((src, dst))), torch.from_numpy(t)
    sei, st, perm = om.stable_time_sort(ei, tt)
    return om.layers_from_temporal(sei, st, n, delta=delta, max_order=K, edge_weight=None if w is None else torch.from_numpy(w)[perm])


def _equal_layers(model, want, keys=("edge_index", "edge_weight", "node_sequence", "inverse_idx"), layers=None):
    for k in (layers or want):
        d = model.layers[k].data
        assert d.num_nodes == want[k]["num_nodes"], k
        for key in keys:
            assert torch.equal(d[key].cpu(), want[k][key]), (k, key)


@pytest.mark.parametrize("route,K", [("levels", 3), ("levels", 4), ("generic", 4)])
def test_fractional_weights_on_long_runs_are_summed_left_to_right(pp, route, K):
    # level by level: k_mo_sums1 / k_mo_sums1_long (layer 1), k_mo_types_wave (the 200-chain: a run of children over four 64-slot rounds,
    # the o_acc carry) and k_mo_types_big (513, 4000) above; generic: k_coalesce_fill / k_coalesce_long_runs on every layer
    src, dst, t, w, n, delta = _long_run_stream(31)
    want = _oracle(src, dst, t, n, delta, K, w)
    model = _build(pp, _graph(pp, src, dst, t, n, w), delta, route, K)
    assert sorted(model.layers) == sorted(want)
    counts = {k: int(want[k]["edge_index"].size(1)) for k in want}
    assert all(counts[k] > 0 for k in want)
    _equal_layers(model, want)


def _hub_bound_check(got, want, count):
    """|got - sum| <= (len - 1) 2^-24 sum|w| per merged edge (sum: the float64 evaluation; positive weights, so sum|w| = sum)."""
    exact = want.double()
    bound = (count.double() - 1).clamp(min=0) * 2.0 ** -24 * exact
    err = (got.double() - exact).abs()
    assert bool((err <= bound).all()), f"max excess {float((err - bound).max()):.3e}"


def test_fractional_weights_on_long_runs_order2_builder(pp):
    # the order-2 builder: layer 1 (k_db2_out; k_db2_hub_out_runs for nodes with more than 64 out-events) left to right, bit for bit.  Layer 2
    # through hub nodes sums in (in-event, task) order: bit for bit for integer-valued weights (next test), within the rounding bound of a
    # reassociated fp32 sum otherwise (the _hip.debruijn2 docstring); every other tensor bit for bit
    src, dst, t, w, n, delta = _long_run_stream(31)
    want = _oracle(src, dst, t, n, delta, 2, w)
    exact = _oracle(src, dst, t, n, delta, 2, w.astype(np.float64))
    runs = _oracle(src, dst, t, n, delta, 2)                        # unit weights: the number of instances of every merged edge
    model = _build(pp, _graph(pp, src, dst, t, n, w), delta, "order2", 2)
    _equal_layers(model, want, layers=(1,))
    _equal_layers(model, want, keys=("edge_index", "node_sequence", "inverse_idx"), layers=(2,))
    got = model.layers[2].data.edge_weight.cpu()
    _hub_bound_check(got, exact[2]["edge_weight"], runs[2]["edge_weight"])
    _hub_bound_check(want[2]["edge_weight"], exact[2]["edge_weight"], runs[2]["edge_weight"])
    print(f" [order-2 builder, layer 2: {int((got != want[2]['edge_weight']).sum())} of {got.numel()} merged weights differ from the left-to-right sum]")


def test_integer_weights_on_long_runs_order2_builder_bit_for_bit(pp):
    src, dst, t, _, n, delta = _long_run_stream(31)
    w = np.random.default_rng(2).integers(1, 9, src.size).astype(np.float32)
    want = _oracle(src, dst, t, n, delta, 2, w)
    assert float(want[2]["edge_weight"].max()) < TWO24
    _equal_layers(_build(pp, _graph(pp, src, dst, t, n, w), delta, "order2", 2), want)


# ------------------------------------------------------------------ B: merged weights past 2^24
def _with_continuations(src, dst, t, n0):
    """A short chain on nodes of its own (n0 .. n0+3, 3 events per hop, delta 10) so that layers 2 and 3 have edges: the fast builders
    hand back a stream with an empty layer."""
    i = np.arange(3)
    src = np.concatenate([src] + [np.full(3, n0 + h) for h in range(3)])
    dst = np.concatenate([dst] + [np.full(3, n0 + h + 1) for h in range(3)])
    t = np.concatenate([t] + [40 * i + 10 * h for h in range(3)])
    return src, dst, t, n0 + 4


def _same_layers(a, b, layers):
    for k in layers:
        x, y = a.layers[k].data, b.layers[k].data
        assert x.num_nodes == y.num_nodes, k
        for key in ("edge_index", "edge_weight", "node_sequence", "inverse_idx"):
            assert torch.equal(x[key], y[key]), (k, key)


def test_unit_weights_past_2_24_in_layer_one(pp):
    # one node pair with 2^24 + 3 events: every route writes float32(2^24 + 3) = 16777220.0 (the reference's sum of ones: 16777216.0)
    L = TWO24 + 3
    src, dst, t, n = _with_continuations(np.zeros(L, np.int64), np.ones(L, np.int64), np.arange(L, dtype=np.int64) % 1000 + 1000, 2)
    n = 10_000               # (unused node ids: the order-2 builder takes streams of at most 2048 events per node)
    g = _graph(pp, src, dst, t, n)
    models = [_build(pp, g, 10, "order2", 2), _build(pp, g, 10, "levels", 3), _build(pp, g, 10, "generic", 3)]
    for model in models:
        d = model.layers[1].data
        assert d.edge_index[:, 0].tolist() == [0, 1]
        assert d.edge_weight[0].item() == float(np.float32(L)) == 16777220.0
    _same_layers(models[0], models[1], (1, 2))
    _same_layers(models[1], models[2], (1, 2, 3))
    del models, g


def test_unit_weights_past_2_24_in_layer_two(pp):
    # bowtie: 4097 events a -> h, then 4097 events h -> c, all inside delta: ONE order-2 edge of 4097^2 = 16785409 instances.  The order-2
    # builder's hub path (h: 4097 in- and out-events), the level-by-level builder (a type with 16785409 children: it hands back) and the
    # generic kernels all write float32(16785409) = 16785408.0; the reference (oracle) sums ones to 16777216.0 - the only difference
    from oracle import model as om
    s = 4097
    src = np.concatenate((np.zeros(s, np.int64), np.ones(s, np.int64)))
    dst = np.concatenate((np.ones(s, np.int64), np.full(s, 2, np.int64)))
    t = np.arange(2 * s, dtype=np.int64)
    n, delta = 64, 10 ** 5
    g = _graph(pp, src, dst, t, n)
    models = [_build(pp, g, delta, "order2", 2), _build(pp, g, delta, "handed_back", 3), _build(pp, g, delta, "generic", 2)]
    want = _oracle(src, dst, t, n, delta, 2)
    assert want[2]["edge_weight"].tolist() == [16777216.0]
    for model in models:
        d2 = model.layers[2].data
        assert d2.edge_weight.tolist() == [16785408.0] == [float(np.float32(s * s))]
        for key in ("edge_index", "node_sequence", "inverse_idx"):
            assert torch.equal(d2[key].cpu(), want[2][key]), key
        _equal_layers(model, want, layers=(1,))
    assert models[1].layers[3].m == 0
    _same_layers(models[0], models[1], (1, 2))
    _same_layers(models[1], models[2], (1, 2))
    del models, g


def test_unit_weights_past_2_24_direct_aggregation(pp):
    # aggregate_edge_index without weights: a merged edge of 2^24 + 5 copies weighs float32(2^24 + 5) = 16777220.0 (reference: 16777216.0)
    L = TWO24 + 5
    ei = torch.zeros((2, L + 2), dtype=torch.int64, device=DEV)
    ei[1, :L] = 1
    ei[0, L] = 1                                        # (two more edges, 1 -> 0 and 1 -> 2)
    ei[:, L + 1] = torch.tensor([1, 2])
    seq = torch.arange(3, device=DEV).unsqueeze(1)
    d = pp.algorithms.aggregate_edge_index(ei, seq).data
    assert d.edge_index.tolist() == [[0, 1, 1], [1, 0, 2]]
    assert d.edge_weight.tolist() == [float(np.float32(L)), 1.0, 1.0] == [16777220.0, 1.0, 1.0]


def test_integer_weights_past_2_24_are_within_1e6_of_the_float64_sum(pp):
    # weight-3.0 events on one node pair, 3 * 5 700 000 > 2^24: PyG's left-to-right fp32 sum drifts by percent past 2^24 (every add rounds
    # up by one), every route is within 1e-6 of the float64 sum (the rule of tests/test_gpu_api.py's fuzz test)
    L = 5_700_000
    src, dst, t, n = _with_continuations(np.zeros(L, np.int64), np.ones(L, np.int64), np.arange(L, dtype=np.int64) % 1000 + 1000, 2)
    n = 10_000
    w = np.full(src.size, 3.0, np.float32)
    g = _graph(pp, src, dst, t, n, w)
    exact = 3.0 * L
    assert exact > TWO24
    for route, K in (("order2", 2), ("levels", 3), ("generic", 3)):
        d = _build(pp, g, 10, route, K).layers[1].data
        assert d.edge_index[:, 0].tolist() == [0, 1]
        assert abs(d.edge_weight[0].item() - exact) <= 1e-6 * exact, (route, d.edge_weight[0].item())
        assert d.edge_weight[1:].tolist() == [9.0] * (d.edge_weight.numel() - 1)
    del g


# ------------------------------------------------------------------ C: counts past 2^31
B31 = 46_341                                    # 46341^2 = 2147488281 = 2^31 + 4633


def _bowtie(pp, s, n=64):
    """s events a=0 -> h=1 at times 0 .. s-1, then s events h -> c=2 at times s .. 2s-1: with delta = 2s every event a -> h continues every
    event h -> c, s^2 order-2 instances of ONE order-2 edge.  (n: node ids beyond 2 unused, for the order-2 builder's events-per-node rule)"""
    src = np.concatenate((np.zeros(s, np.int64), np.ones(s, np.int64)))
    dst = np.concatenate((np.ones(s, np.int64), np.full(s, 2, np.int64)))
    return _graph(pp, src, dst, np.arange(2 * s, dtype=np.int64), n), 2 * s


def test_temporal_lift_past_2_31_pairs(pp):
    # lift_order_temporal: E2 = 2147488281 pairs (i, s + j) in lexicographic order; the int64 slots beyond 2^31 of the expansion
    s = B31
    g, delta = _bowtie(pp, s)
    eg = pp.algorithms.lift_order_temporal(g, delta)
    e2 = s * s
    assert e2 > TWO31 and tuple(eg.shape) == (2, e2)
    step = 1 << 28
    cont = torch.zeros(s, dtype=torch.int64, device=DEV)
    last = -1
    for lo in range(0, e2, step):                   # every slot, a chunk at a time: slot q holds (q // s, s + q % s)
        hi = min(lo + step, e2)
        src = eg[0, lo:hi]
        assert int(src[0]) >= last and bool((src[1:] >= src[:-1]).all()), lo              # non-decreasing sources
        last = int(src[-1])
        cont += torch.bincount(src, minlength=s)
        q = torch.arange(lo, hi, device=DEV, dtype=torch.int64)
        assert torch.equal(src, q // s) and torch.equal(eg[1, lo:hi], s + q % s), lo
        del q, src
    assert int(cont.min()) == int(cont.max()) == s                   # every source has s continuations
    rng = np.random.default_rng(0)
    slots = [TWO31 - 1, TWO31, TWO31 + 1, e2 - 1] + rng.integers(0, e2, 300).tolist()
    for q in slots:
        assert (int(eg[0, q]), int(eg[1, q])) == (q // s, s + q % s), q
    del eg, g


def _refused_at_2_31(pp, monkeypatch, g, delta, K):
    """from_temporal_graph(max_order=K) on a stream with 2^31 or more instances at some order: the level-by-level builder hands back
    (``_hip.multi_order_temporal`` -> None), ONE generic build runs and ends in a HipError that names 2^31 — never in layers."""
    from pathpyg_amd import _hip
    from pathpyg_amd._lib import HipError
    from pathpyg_amd.core import multi_order_model as mm
    fast, generic = [], []
    real_fast, real_generic = _hip.multi_order_temporal, mm.MultiOrderModel._from_temporal_graph_generic

    def fast_counted(*args, **kw):
        out = real_fast(*args, **kw)
        fast.append(out is None)
        return out

    def generic_counted(*args):
        generic.append(args[2])
        return real_generic(*args)

    monkeypatch.setattr(_hip, "multi_order_temporal", fast_counted)
    monkeypatch.setattr(mm.MultiOrderModel, "_from_temporal_graph_generic", staticmethod(generic_counted))
    with pytest.raises(HipError, match=r"2\^31") as err:
        pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=K)
    msg = str(err.value)
    del err                                        # (the traceback holds the frames' device tensors)
    monkeypatch.undo()
    return fast, generic, msg


def test_bowtie_past_2_31_with_max_order_three_is_refused(pp, monkeypatch):
    # level 1: (a, h) has 46341 events of 46341 continuations each: k_mo_sums1_long's int64 count sets kMoOverflow, the builder hands back;
    # the generic kernels lift 2147488281 order-2 instances and refuse to coalesce them
    g, delta = _bowtie(pp, B31)
    fast, generic, msg = _refused_at_2_31(pp, monkeypatch, g, delta, 3)
    assert fast == [True] and generic == [3], (fast, generic, msg)
    del g


def test_bowtie_past_2_31_with_max_order_two(pp, monkeypatch):
    # the order-2 builder: A2 = 1, E2 = 2147488281 through the hub node h (k_db2_hubx: one order-2 edge of more than 2^31 instances, an
    # unsigned count).  The builder must KEEP the stream and give the analytic layers: a hand-back fails the test
    from pathpyg_amd import _hip
    s = B31
    g, delta = _bowtie(pp, s)
    kept = []
    real = _hip.debruijn2

    def counted(*args, **kw):
        out = real(*args, **kw)
        kept.append(out is not None)
        return out

    monkeypatch.setattr(_hip, "debruijn2", counted)
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=2)
    monkeypatch.undo()
    assert kept == [True], "the order-2 builder handed the bowtie back"
    assert getattr(model, "_pp_fused", None) is not None and model.sizes["E2"] == s * s and model.sizes["A2"] == 1
    d1, d2 = model.layers[1].data, model.layers[2].data
    assert d1.edge_index.tolist() == [[0, 1], [1, 2]] and d1.edge_weight.tolist() == [float(s), float(s)]
    assert d2.edge_index.tolist() == [[0], [1]]
    assert d2.edge_weight.tolist() == [2147488256.0] == [float(np.float32(s * s))]
    assert d2.node_sequence.tolist() == [[0, 1], [1, 2]]
    assert torch.equal(d2.inverse_idx.cpu(), torch.cat((torch.zeros(s, dtype=torch.int64), torch.ones(s, dtype=torch.int64))))
    del model, g


def test_bowtie_past_2_32_with_max_order_two_is_handed_back(pp, monkeypatch):
    # 65536 x 65536 bowtie: its one order-2 edge has 2^32 instances, which k_db2_hubx's 32-bit count of an edge cannot hold (it would wrap to
    # 0 and drop the edge): the builder reports it and hands the stream back.  (The generic kernels would refuse it as above after a 68 GB
    # lift: here a stand-in records the call instead)
    from pathpyg_amd import _hip
    from pathpyg_amd.core import multi_order_model as mm
    g, delta = _bowtie(pp, 1 << 16)
    kept, generic = [], []
    real = _hip.debruijn2

    def counted(*args, **kw):
        out = real(*args, **kw)
        kept.append(out is not None)
        return out

    class HandedBack(Exception):
        pass

    def stand_in(*args):
        generic.append(args[2])
        raise HandedBack

    monkeypatch.setattr(_hip, "debruijn2", counted)
    monkeypatch.setattr(mm.MultiOrderModel, "_from_temporal_graph_generic", staticmethod(stand_in))
    with pytest.raises(HandedBack):
        pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=2)
    monkeypatch.undo()
    assert kept == [False] and generic == [2], (kept, generic)
    del g


@pytest.mark.parametrize("parents,tail", [(4096, 1 << 19), (256, 1 << 23)], ids=["4096x2^19", "256x2^23"])
def test_level_three_past_2_31_instances_is_refused(pp, monkeypatch, parents, tail):
    # `parents` events a -> b, one b -> h, then `tail` events h -> c, all inside delta: parents * tail = 2^31 level-3 instances.  The
    # level-by-level builder refuses at its level-2 step: the node pair (b, h) has one event of `tail` > kMoBigMax continuations, so
    # k_mo_children_big sets kMoOverflow (the int64 children counts of k_mo_types* are defensive: with kMoBigMax^2 < 2^31 no stream reaches
    # them first).  The generic kernels then lift exactly 2^31 line-graph pairs (int64 slots) and refuse to coalesce them
    assert parents * tail == TWO31
    src = np.concatenate((np.zeros(parents, np.int64), [1], np.full(tail, 2, np.int64)))
    dst = np.concatenate((np.ones(parents, np.int64), [2], np.full(tail, 3, np.int64)))
    m = src.size
    g = _graph(pp, src, dst, np.arange(m, dtype=np.int64), 64)
    fast, generic, msg = _refused_at_2_31(pp, monkeypatch, g, m, 3)
    assert fast == [True] and generic == [3], (fast, generic, msg)
    del g
