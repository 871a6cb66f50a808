"""Timestamp order and window logic on non-finite float64 times (cases: tests/time_domain_cases.py, pinned on the CPU by
test_time_domain_host.py): the time sort, the sortedness check and the three window searches — ``k_temporal_count`` with its per-wave
marks (csrc/pp_lift.hip), the per-node searches of the fused order-2 builder (csrc/pp_debruijn.hip) and ``pp_temporal_windows`` under
the level-by-level builder (csrc/pp_multiorder.hip) — on NaNs of both signs, infinities, signed zeros, subnormals, values beyond 2^53
and thresholds ``t + delta`` that saturate at inf or become NaN.

The contract ("Timestamp order"): events are ordered as ``torch.sort(time, stable=True)`` orders them — ascending,
``-0.0 == 0.0``, every NaN last and tied with every other NaN, ties in input order; a NaN event is neither a source nor a continuation,
a NaN threshold admits nothing.  Every comparison is exact (``torch.equal``; times by their bit patterns): event weights are
integer-valued float32, so merged sums are exact in any association."""
import pathlib

import numpy as np
import pytest
import torch

from test_gpu_builder import _build, _compare
from tests import time_domain_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "time_domain_vectors.npz"
INT64_MIN = -(2 ** 63)


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from pathpyg_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def cu(x):
    return x.to(DEV)


def _pool_cycle(n):
    pool = tc.special_pool()
    return torch.from_numpy(pool[np.arange(n) % len(pool)])


# ---------------------------------------------------------------- sort primitives
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 100_003])
def test_argsort_orders_the_pool_like_torch(hip, n):
    t = _pool_cycle(n)
    assert torch.equal(hip.argsort(cu(t)).cpu(), tc.torch_order(t))


@pytest.mark.parametrize("kind", ["all-nan", "zeros", "equal", "nan-signs-around-inf"])
def test_argsort_ties_keep_their_input_order(hip, kind):
    n = 4099                                                      # two sort tiles
    if kind == "all-nan":                                         # both signs, many payloads: ONE tie
        raw = np.where(np.arange(n) % 2 == 0, 0x7FF8000000000000, 0xFFF8000000000000).astype(np.uint64) + (np.arange(n) % 7).astype(np.uint64)
        t = torch.from_numpy(raw.view(np.float64).copy())
        assert bool(torch.isnan(t).all())
    elif kind == "zeros":
        t = torch.from_numpy(np.where(np.arange(n) % 2 == 0, -0.0, 0.0))
    elif kind == "equal":
        t = torch.full((n,), 2.0 ** 53 + 2, dtype=torch.float64)
    else:                                                         # sign-bit NaNs must not land below -inf
        t = torch.from_numpy(np.array([tc.NAN_MINUS, tc.INF, tc.NAN_PLUS, -tc.INF, tc.NAN_MINUS, 0.0] * 700))
    want = tc.torch_order(t)
    if kind != "nan-signs-around-inf":
        assert torch.equal(want, torch.arange(t.numel()))
    assert torch.equal(hip.argsort(cu(t)).cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_argsort_of_narrow_floats(hip, dtype):
    t = _pool_cycle(4097).to(dtype)                               # out-of-range values become +-inf, tiny ones zeros of either sign
    assert bool(torch.isnan(t).any()) and bool(torch.isinf(t).any())
    assert torch.equal(hip.argsort(cu(t)).cpu(), tc.torch_order(t))


DESCENT_CASES = [[5.0, tc.NAN, 1.0], [tc.NAN, 1.0], [1.0, tc.NAN], [1.0, tc.NAN, tc.NAN], [-0.0, 0.0, -0.0], [tc.INF, tc.INF],
                 [-tc.INF, 1.0, tc.INF, tc.NAN], [5.0, float(tc.NAN_MINUS), 1.0], [float(tc.NAN_MINUS), tc.NAN, float(tc.NAN_MINUS)]]


def _value_id(v):
    return ("-nan" if np.signbit(v) else "nan") if np.isnan(v) else repr(float(v))


@pytest.mark.parametrize("case", DESCENT_CASES, ids=[",".join(_value_id(v) for v in c) for c in DESCENT_CASES])
def test_descent_count_is_zero_exactly_on_torch_sorted_vectors(hip, case):
    t = torch.from_numpy(np.array(case, dtype=np.float64))
    is_sorted = torch.equal(tc.torch_order(t), torch.arange(t.numel()))
    assert hip.is_sorted(cu(t)) == is_sorted
    assert (hip.time_stats(cu(t))[0] == 0) == is_sorted


def test_descents_across_wave_and_block_borders(hip):
    """One NaN in front of a number at every position of a long sorted vector's first 600 entries: each is one descent."""
    base = torch.arange(5000, dtype=torch.float64)
    for at in (0, 62, 63, 64, 255, 256, 511, 4998):
        t = base.clone()
        t[at] = float(tc.NAN_MINUS) if at % 2 else tc.NAN
        assert not hip.is_sorted(cu(t)), at
        assert hip.time_stats(cu(t))[0] >= 1, at
    t = base.clone()
    t[-1] = tc.NAN                                                  # at the very end it is in place
    assert hip.is_sorted(cu(t)) and hip.time_stats(cu(t))[0] == 0


def test_gather_events_moves_the_time_bits(hip):
    ei, t, _ = tc.pool_stream()
    perm = hip.argsort(cu(t))
    assert torch.equal(perm.cpu(), tc.torch_order(t))
    got_ei, got_t = hip.gather_events(cu(ei), cu(t), perm)
    assert torch.equal(tc.bits(got_t.cpu()), tc.bits(t[perm.cpu()]))
    assert torch.equal(got_ei.cpu(), ei[:, perm.cpu()])


@pytest.mark.parametrize("n", [3, 4097, 300_001])
def test_sort_pairs_u64_over_the_full_64_bit_range(hip, n):
    g = torch.Generator().manual_seed(n)
    halves = torch.randint(0, 2 ** 32, (2, n), generator=g, dtype=torch.int64)
    keys = (halves[0] << 32) | halves[1]                                       # all of int64: the high half wraps into the sign bit
    keys[0], keys[n // 2], keys[-1] = -1, INT64_MIN, 2 ** 63 - 1              # 0xFF..FF, 0x80..00, 0x7F..FF
    assert int((keys < 0).sum()) > 0 and int((keys >= 2 ** 62).sum()) > 0
    ks, vs = hip.sort_pairs(cu(keys), None, 0, 64)
    order = torch.sort(keys ^ INT64_MIN, stable=True)                          # unsigned order of the bit patterns
    assert torch.equal(vs.cpu().long(), order.indices)
    assert torch.equal(ks.cpu(), keys[order.indices])


# ---------------------------------------------------------------- TemporalGraph construction
@pytest.mark.parametrize("name", ["pool", "mixed"])
def test_temporal_graph_sorts_like_torch(pp, name):
    ei, t, n = tc.pool_stream() if name == "pool" else tc.mixed_stream(1)
    m = t.numel()
    perm = tc.torch_order(t)
    w, label = tc.weights(m), np.arange(m) * 3 + 1
    data = pp.Data(edge_index=cu(ei), time=cu(t), num_nodes=n)
    data["edge_weight"] = cu(w)
    data["edge_label"] = label.copy()
    g = pp.TemporalGraph(data)

    def check(graph):
        d = graph.data
        assert torch.equal(tc.bits(d.time.cpu()), tc.bits(t[perm]))
        assert torch.equal(d.edge_index.cpu(), ei[:, perm])
        assert torch.equal(d.edge_weight.cpu(), w[perm])
        assert np.array_equal(d.edge_label, label[perm.numpy()])
    check(g)
    check(pp.TemporalGraph(g.data))                               # already in order: nothing moves


@pytest.mark.parametrize("nan", [tc.NAN_PLUS, tc.NAN_MINUS], ids=["nan", "sign-bit-nan"])
def test_temporal_graph_moves_a_nan_from_the_middle_to_the_end(pp, nan):
    t = torch.from_numpy(np.array([5.0, nan, 1.0]))
    g = pp.TemporalGraph(pp.Data(edge_index=cu(torch.tensor([[0, 1, 2], [1, 2, 0]])), time=cu(t), num_nodes=3))
    assert torch.equal(tc.bits(g.data.time.cpu()), tc.bits(t[torch.tensor([2, 0, 1])]))
    assert g.data.edge_index.cpu().tolist() == [[2, 0, 1], [0, 1, 2]]


# ---------------------------------------------------------------- builder 1: the event-graph lift
@pytest.mark.parametrize("d", tc.DELTAS, ids=tc.DELTA_IDS)
@pytest.mark.parametrize("name", ["pool", "mixed"])
def test_temporal_lift_equals_the_mask_loop(hip, name, d):
    ei, t, n, _ = tc.stream(name)
    want = tc.expected_lift(name, d)
    got = hip.temporal_lift(cu(ei), cu(t), n, tc.delta_tensor(d)).cpu()
    assert got.shape == want.shape, f"{got.size(1)} pairs, the mask loop has {want.size(1)}"
    assert torch.equal(got, want)


def test_temporal_lift_python_float_and_int_deltas(hip):
    ei, t, n, _ = tc.stream("pool")
    for delta, d in ((1.0, 1.0), (0.25, 0.25), (float("inf"), tc.INF), (float("nan"), tc.NAN), (2, 2.0)):
        assert torch.equal(hip.temporal_lift(cu(ei), cu(t), n, delta).cpu(), tc.expected_lift("pool", d)), repr(delta)


def test_temporal_lift_ties_in_front_of_a_nan_tail(hip):
    """The search for the end of a run of ties gallops over the stream: where the run is followed by fewer later numbers than the
    gallop's stride it lands in the NaN tail, which must read as "later than everything" and not send the search past the numbers."""
    for ties, later, nans in ((3, 1, 70), (40, 2, 200), (70, 5, 64), (5, 0, 300)):
        t = torch.tensor([1.0] * ties + [2.0] * later + [tc.NAN] * nans, dtype=torch.float64)
        m = t.numel()
        ei = torch.stack((torch.zeros(m, dtype=torch.long), torch.zeros(m, dtype=torch.long)))       # one node, self loops: every later event continues
        want = tc.mask_loop(ei, t, tc.delta_tensor(1.0))
        assert want.size(1) == ties * later
        assert torch.equal(hip.temporal_lift(cu(ei), cu(t), 1, tc.delta_tensor(1.0)).cpu(), want), (ties, later, nans)


def test_temporal_lift_equals_the_reference_vectors(hip):
    golden = np.load(GOLDEN, allow_pickle=False)
    names = sorted({k.split("/")[1] for k in golden.files})
    assert len(names) == 4
    for name in names:
        ei = torch.from_numpy(golden[f"temporal/{name}/edge_index"])
        t = torch.from_numpy(golden[f"temporal/{name}/time"])
        out = torch.from_numpy(golden[f"temporal/{name}/out"]).long()
        out = out[:, torch.sort(out[0] * ei.size(1) + out[1]).indices]
        got = hip.temporal_lift(cu(ei), cu(t), int(golden[f"temporal/{name}/num_nodes"]), float(golden[f"temporal/{name}/delta"])).cpu()
        assert torch.equal(got, out), name


@pytest.mark.parametrize("d", [1.0, 1.7e308, tc.INF], ids=repr)
def test_temporal_lift_edge_range_shards_reassemble(hip, d):
    from pathpyg_amd.distributed import event_ranges, halo_end
    ei, t, n, _ = tc.stream("pool")
    delta = tc.delta_tensor(d)
    full = tc.expected_lift("pool", d)
    for world in (2, 5):
        parts = []
        for lo, hi in event_ranges(ei.size(1), world):
            end = halo_end(t, hi, delta)
            parts.append(hip.temporal_lift(cu(ei[:, lo:end]), cu(t[lo:end]), n, delta, n_own=hi - lo, id_offset=lo).cpu())
        assert torch.equal(torch.cat(parts, dim=1), full), world


# ---------------------------------------------------------------- the oracle's layers, once per (stream, delta, weighted)
_LAYERS: dict = {}


def _oracle_layers(name, d, weighted, max_order):
    """``oracle.model.layers_from_temporal`` on the mask loop's event graph (what ``loop_lift=True`` computes, handed over so that the
    loop runs once per stream and delta and an empty event graph is no exception)."""
    key = (name, repr(d), weighted, max_order)
    if key not in _LAYERS:
        from oracle import model as om
        ei, t, n, perm = tc.stream(name)
        w = tc.weights(t.numel())[perm] if weighted else None
        _LAYERS[key] = om.layers_from_temporal(ei, t, n, delta=tc.delta_tensor(d), max_order=max_order, edge_weight=w,
                                               event_graph=tc.expected_lift(name, d))
    return _LAYERS[key]


# ---------------------------------------------------------------- builder 2: the fused order-2 builder
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("d", tc.DELTAS, ids=tc.DELTA_IDS)
def test_fused_builder_on_the_pool_stream(hip, d, weighted):
    ei, t, n, perm = tc.stream("pool")
    w = tc.weights(t.numel())[perm] if weighted else None
    delta = tc.delta_tensor(d)
    fused = _build(ei, t, n, delta, w, True)
    _compare(fused, _build(ei, t, n, delta, w, False), hubs=True)
    want = _oracle_layers("pool", d, weighted, 2)
    for k, gs in ((1, fused.fo), (2, fused.ho)):
        plan = gs.plan
        ptr = plan.bwd_ptr.long().cpu()
        src = torch.repeat_interleave(torch.arange(plan.n_src), ptr[1:] - ptr[:-1])
        assert torch.equal(torch.stack((src, plan.bwd_idx.long().cpu())), want[k]["edge_index"]), f"layer {k} edge_index"
    built = hip.debruijn2(cu(ei), cu(t), n, delta, None if w is None else cu(w))
    assert torch.equal(built.fo_weight.cpu(), want[1]["edge_weight"].to(torch.float32))
    assert built.sizes["E2"] == tc.expected_lift("pool", d).size(1)
    assert fused.sizes["E2"] == built.sizes["E2"] and fused.sizes["A2"] == want[2]["edge_index"].size(1)


@pytest.mark.parametrize("d", [0.25, tc.INF, tc.NAN], ids=repr)
def test_fused_builder_on_the_mixed_stream(hip, d):
    ei, t, n, perm = tc.stream("mixed")
    w = tc.weights(t.numel())[perm]
    delta = tc.delta_tensor(d)
    fused = _build(ei, t, n, delta, w, True)
    _compare(fused, _build(ei, t, n, delta, w, False), hubs=True)
    assert fused.sizes["E2"] == tc.expected_lift("mixed", d).size(1)


# ---------------------------------------------------------------- builder 3: the level-by-level builder
MO_BIG = 4096            # continuations of one node sequence the level-by-level builder takes (csrc/pp_multiorder.hip, PP_MO_BIG)


def _level_by_level_applies(name, d):
    """The builder's documented refusals (``_hip.multi_order_temporal``): a layer without edges, a node sequence with more than 4096
    continuations.  The continuations of an order-k node are the instances of its out-edges: the unit-weight sums of the oracle."""
    layers = _oracle_layers(name, d, False, 3)
    for k in (1, 2, 3):
        if layers[k]["edge_index"].size(1) == 0:
            return False
    for k in (2, 3):
        e, w = layers[k]["edge_index"], layers[k]["edge_weight"]
        per_node = torch.zeros(layers[k]["num_nodes"], dtype=torch.float64).index_add_(0, e[0], w.double())
        if float(per_node.max()) > MO_BIG:
            return False
    return True


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("d", tc.DELTAS, ids=tc.DELTA_IDS)
@pytest.mark.parametrize("name", ["pool", "pool24"])
def test_level_by_level_builder(pp, name, d, weighted):
    ei, t, n, perm = tc.stream(name)
    data = pp.Data(edge_index=cu(ei), time=cu(t), num_nodes=n)
    if weighted:
        data["edge_weight"] = cu(tc.weights(t.numel())[perm])
    g = pp.TemporalGraph(data)
    assert torch.equal(tc.bits(g.data.time.cpu()), tc.bits(t))
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=tc.delta_tensor(d), max_order=3)
    applies = _level_by_level_applies(name, d)
    if name == "pool24":                                           # this stream is sized so that only the empty event graphs are handed back
        assert applies == (d > 0)
    assert ("layers" in getattr(model, "sizes", {})) == applies, "level-by-level builder: " + ("did not run" if applies else "ran on a stream it documents to refuse")
    want = _oracle_layers(name, d, weighted, 3)
    assert sorted(model.layers) == [1, 2, 3]
    for k in (1, 2, 3):
        layer = model.layers[k].data
        assert torch.equal(layer.edge_index.cpu(), want[k]["edge_index"]), f"layer {k} edge_index"
        assert torch.equal(layer.edge_weight.cpu(), want[k]["edge_weight"].to(torch.float32)), f"layer {k} edge_weight"


# ---------------------------------------------------------------- sortedness guards
def _nan_in_the_middle(name, nan):
    ei, t, n, _ = tc.stream(name)
    at = t.numel() // 2
    assert bool(torch.isfinite(t[at - 1])) and bool(torch.isfinite(t[at + 1])) and bool(t[at - 1] <= t[at + 1])
    raw = t.numpy().copy()
    raw[at] = nan
    t = torch.from_numpy(raw)
    assert int(tc.bits(t)[at]) == int(np.array([nan]).view(np.int64)[0])
    return ei, t, n


@pytest.mark.parametrize("nan", [tc.NAN_PLUS, tc.NAN_MINUS], ids=["nan", "sign-bit-nan"])
def test_a_nan_in_the_middle_is_not_sorted_by_time(hip, nan):
    delta = tc.delta_tensor(1.0)
    ei, t, n = _nan_in_the_middle("pool", nan)
    with pytest.raises(ValueError, match="not sorted by time"):
        hip.temporal_lift(cu(ei), cu(t), n, delta)
    with pytest.raises(ValueError, match="not sorted by time"):
        hip.debruijn2(cu(ei), cu(t), n, delta, None)
    ei24, t24, n24 = _nan_in_the_middle("pool24", nan)
    with pytest.raises(ValueError, match="not sorted by time"):
        hip.multi_order_temporal(cu(ei24), cu(t24), n24, delta, None, 3)
    # the same events with the NaN where torch puts it: accepted, and the results are the mask loop's
    for (e, x, k) in ((ei, t, n), (ei24, t24, n24)):
        perm = tc.torch_order(x)
        e, x = e[:, perm].contiguous(), x[perm].contiguous()
        want = tc.mask_loop(e, x, delta)
        assert torch.equal(hip.temporal_lift(cu(e), cu(x), k, delta).cpu(), want)
        assert hip.debruijn2(cu(e), cu(x), k, delta, None).sizes["E2"] == want.size(1)
        built = hip.multi_order_temporal(cu(e), cu(x), k, delta, None, 3)
        if k == n24:
            assert built is not None and built[1].n_instances == want.size(1)
