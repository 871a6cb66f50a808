"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol of include/pathpyg_amd.h,
host containers behave like the reference's, and compute entry points fail loudly without a GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import pathpyg_amd as pp
from pathpyg_amd import _hip, _lib

NO_GPU = not torch.cuda.is_available()


def test_library_exports_every_declared_symbol():
    protos = _lib.declared_functions()
    text = re.sub(r"/\*.*?\*/", " ", _lib.HEADER.read_text(), flags=re.S)
    names_in_header = set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", text))
    assert names_in_header == set(protos), "header parser missed a declaration"
    assert len(protos) >= 40
    handle = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert handle.pp_version() == 100
    assert isinstance(handle.pp_last_error(), bytes)
    # size queries are pure host code: callable without a GPU
    assert handle.pp_temporal_ws_bytes(1000, 10) > 0
    assert handle.pp_sort_ws_bytes(4096, 4) >= 4096 * 8
    assert handle.pp_weight_grad_ws_bytes(1000, 64, 64) >= 64 * 64 * 4
    assert handle.pp_gcn_plan_ws_bytes(100, 10) > 0
    # the {size, status} header of a workspace sits at its start: the accessors are host-side pointer casts
    buf = ctypes.create_string_buffer(64)
    for accessor in (handle.pp_lift_result_ptr, handle.pp_aggregate_result_ptr, handle.pp_plan_result_ptr):
        got = accessor(ctypes.cast(buf, ctypes.c_void_p))
        assert ctypes.cast(got, ctypes.c_void_p).value == ctypes.addressof(buf)


def test_library_is_a_plain_c_abi_without_torch():
    # the .so must not link torch / c10: it is a C ABI over HIP only
    # (static DT_NEEDED entries: `ldd` would also print where the loader FINDS libamdhip64, which may be torch's bundled copy)
    import subprocess
    out = subprocess.run(["readelf", "-d", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    needed = [line.split("[")[1].split("]")[0] for line in out.splitlines() if "(NEEDED)" in line]
    assert any(lib.startswith("libamdhip64") for lib in needed), needed
    assert not any("torch" in lib or "c10" in lib for lib in needed), needed


@pytest.mark.skipif(not NO_GPU, reason="checks the no-GPU failure mode")
def test_compute_entry_points_fail_loudly_without_gpu():
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="MI355X"):
        pp.algorithms.lift_order_edge_index(ei, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        pp.algorithms.aggregate_node_attributes(ei, torch.ones(3), "src")
    with pytest.raises(RuntimeError, match="MI355X"):
        pp.Graph.from_edge_list([("a", "b"), ("b", "c")])
    with pytest.raises(RuntimeError, match="MI355X"):
        pp.TemporalGraph.from_edge_list([("a", "b", 2), ("b", "c", 1)])
    with pytest.raises(RuntimeError):
        _hip.temporal_lift(ei, torch.tensor([1, 2]), 3, 1)
    with pytest.raises(ValueError):                               # argument errors come first, like the reference
        pp.algorithms.aggregate_node_attributes(ei, torch.ones(3), "unknown")
    w = torch.nn.Parameter(torch.ones(4))                         # the optimizer has no CPU path either
    w.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="MI355X"):
        pp.nn.optim.Adam([w], lr=1e-3).step()
    assert torch.equal(w.detach(), torch.ones(4))
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):                           # same argument checks as torch.optim.Adam
            pp.nn.optim.Adam([w], **bad)


def test_event_stream_normaliser():
    # the checks temporal_lift, debruijn2, multi_order_temporal and debruijn2_part_count share: device-agnostic, so plain CPU tensors here
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]])
    time, w = _hip._event_stream(ei, torch.tensor([3, 1, 2], dtype=torch.int16))
    assert time.dtype == torch.int64 and time.tolist() == [3, 1, 2] and w is None
    w32 = torch.arange(6, dtype=torch.float32)[::2]
    time, w = _hip._event_stream(ei, torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64), w32)
    assert time.dtype == torch.float64 and w.is_contiguous() and torch.equal(w, w32)
    with pytest.raises(TypeError, match="int64 or float64"):
        _hip._event_stream(ei, torch.tensor([1.0, 2.0, 3.0]), w32)
    with pytest.raises(ValueError, match="number of events"):
        _hip._event_stream(ei, torch.tensor([1, 2]))
    assert _hip._event_stream(ei, torch.tensor([1, 2, 3]), torch.ones(3, dtype=torch.float64)) is None      # does not apply
    assert _hip._event_stream(ei, torch.tensor([1, 2, 3]), torch.ones(2)) is None
    # the callers look at the device first: a host stream is the "no CPU path" error, not a dtype error
    for call in (lambda t: _hip.temporal_lift(ei, t, 3, 1), lambda t: _hip.debruijn2(ei, t, 3, 1),
                 lambda t: _hip.multi_order_temporal(ei, t, 3, 1, None, 3)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(torch.tensor([1.0, 2.0, 3.0]))


def test_delta_resolution_follows_torch_promotion():
    i64, f64 = torch.int64, torch.float64
    assert _hip.resolve_delta(i64, 5) == (_hip.DELTA_I64, 5, 0.0)
    kind, _, df = _hip.resolve_delta(i64, 0.1)
    assert kind == _hip.DELTA_F32 and df == float(np.float32(0.1))           # python float -> float32 tensor
    assert _hip.resolve_delta(i64, np.float64(0.1)) == (_hip.DELTA_F64, 0, 0.1)
    assert _hip.resolve_delta(f64, 3) == (_hip.DELTA_F64, 0, 3.0)
    assert _hip.resolve_delta(f64, 0.1)[2] == float(np.float32(0.1))          # float32-rounded, then widened
    assert _hip.resolve_delta(f64, np.float64(0.1))[2] == 0.1
    with pytest.raises(ValueError):
        _hip.resolve_delta(i64, torch.tensor([1, 2]))


def test_data_bag():
    d = pp.Data(edge_index=torch.tensor([[0, 1, 1], [1, 2, 0]]), edge_weight=torch.ones(3), node_size=torch.zeros(4), num_nodes=4,
                time=torch.tensor([3, 1, 2]))
    assert d.num_nodes == 4 and d.num_edges == 3
    assert "edge_weight" in d and "x" not in d and d.x is None and d.y is None
    with pytest.raises(AttributeError):
        d.not_there
    assert set(d.keys()) == {"edge_index", "edge_weight", "node_size", "num_nodes", "time"}
    assert d.is_edge_attr("edge_weight") and d.is_edge_attr("edge_index") and d.is_edge_attr("time")
    assert d.is_node_attr("node_size") and not d.is_node_attr("edge_weight")
    d["foo"] = 3
    d.bar = torch.ones(2)
    assert d.foo == 3 and d["bar"].tolist() == [1.0, 1.0]
    d.foo = None
    assert "foo" not in d
    inferred = pp.Data(edge_index=torch.tensor([[0, 5], [1, 2]]))
    assert inferred.num_nodes == 6
    c = d.clone()
    c.edge_weight[0] = 7
    assert d.edge_weight[0] == 1


def test_index_map_matches_reference_behaviour():
    m = pp.IndexMap(["A", "C", "B"])
    assert str(m) == "A -> 0\nC -> 1\nB -> 2\n"
    assert m.to_idx("C") == 1 and m.to_id(2) == "B" and m.num_ids() == 3 and m.has_ids
    assert m.to_ids([0, 2]).tolist() == ["A", "B"]
    assert m.to_idxs([["A", "B"], ["B", "C"]]).tolist() == [[0, 2], [2, 1]]
    m.add_id("D")
    assert m.to_idx("D") == 3
    m.add_ids(["F", "E"])
    assert m.to_idx("E") == 5
    with pytest.raises(ValueError):
        m.add_id("A")
    with pytest.raises(ValueError):
        pp.IndexMap(["a", "a"])
    h = pp.IndexMap([("A", "B"), ("A", "C"), ("B", "C")])
    assert h.id_shape == (-1, 2) and h.to_id(1) == ("A", "C") and h.to_idx(("B", "C")) == 2
    assert h.to_ids([[0], [2]]).shape == (2, 1, 2)
    assert h.to_idxs([("A", "B"), ("B", "C")]).tolist() == [0, 2]
    e = pp.IndexMap()
    assert not e.has_ids and e.num_ids() == 0 and e.to_idx(7) == 7 and e.to_id(3) == 3
    assert e.to_idxs([1, 0]).tolist() == [1, 0]
    # lazy higher-order map = what reference multi_order_model.py:119 builds with a Python loop
    lazy = pp.IndexMap.from_node_sequence(pp.IndexMap(list("abcd")), torch.tensor([[0, 1], [2, 3], [1, 1]]))
    eager = pp.IndexMap([("a", "b"), ("c", "d"), ("b", "b")])
    assert lazy.num_ids() == 3 and lazy.to_id(1) == eager.to_id(1) and lazy.to_idx(("b", "b")) == eager.to_idx(("b", "b"))
    assert str(lazy) == str(eager)
    assert pp.IndexMap.from_node_sequence(pp.IndexMap(), torch.tensor([[4, 5]])).to_id(0) == (4, 5)


def test_path_data_layout_matches_oracle():
    from oracle import model as om
    walks = [[0, 2, 3], [1, 2, 4, 0], [3, 3]]
    weights = [2.0, 1.0, 4.0]
    p = pp.PathData()
    p.append_walk(walks[0], weights[0])
    p.append_walks(walks[1:], weights[1:])
    ref = om.walks_to_path_tensors(walks, weights)
    for key in ("edge_index", "node_sequence", "dag_weight", "dag_num_edges", "dag_num_nodes"):
        assert torch.equal(p.data[key], ref[key]), key
    assert p.num_paths == 3 and p.data.num_nodes == 9
    assert p.get_walk(1) == (1, 2, 4, 0)
    assert str(p) == "PathData with 3 paths with total weight 7.0"
    named = pp.PathData(pp.IndexMap(list("ABCDE")))
    named.append_walk(("A", "C", "D"), weight=2.0)
    assert named.get_walk(0) == ("A", "C", "D") and named.map_node_seq([0, 2]) == ["A", "C"]


def test_multi_order_model_shell():
    m = pp.MultiOrderModel()
    assert m.layers == {} and str(m) == "MultiOrderModel with max. order 0"
    m.layers[5] = "x"
    assert str(m) == "MultiOrderModel with max. order 5"
    with pytest.raises(ValueError):
        pp.MultiOrderModel().to_dbgnn_data(max_order=2)


def test_dbgnn_module_state_dict_layout():
    net = pp.nn.DBGNN(num_classes=3, num_features=(7, 9), hidden_dims=[16, 32, 8], p_dropout=0.4)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert shapes == {
        "higher_order_layers.0.bias": (16,), "higher_order_layers.0.lin.weight": (16, 9),
        "higher_order_layers.1.bias": (32,), "higher_order_layers.1.lin.weight": (32, 16),
        "first_order_layers.0.bias": (16,), "first_order_layers.0.lin.weight": (16, 7),
        "first_order_layers.1.bias": (32,), "first_order_layers.1.lin.weight": (32, 16),
        "bipartite_layer.lin1.weight": (8, 32), "bipartite_layer.lin1.bias": (8,),
        "bipartite_layer.lin2.weight": (8, 32), "bipartite_layer.lin2.bias": (8,),
        "lin.weight": (3, 8), "lin.bias": (3,),
    }
    from oracle import dbgnn as od
    net.load_state_dict(od.init_params(3, (7, 9), [16, 32, 8]))          # oracle parameter dict == state_dict layout
    assert float(net.first_order_layers[0].bias.abs().sum()) == 0.0


def test_dbgnn_hints_are_bound_to_the_tensors_they_describe():
    """hints of to_dbgnn_data must not survive a replaced or edited edge index."""
    from pathpyg_amd.nn.dbgnn import _valid_hints
    ei = torch.tensor([[0, 1], [1, 2]])
    w = torch.ones(2)
    d = pp.Data(num_nodes=3, num_ho_nodes=2, edge_index=ei, edge_weights=w, edge_index_higher_order=ei.clone(), edge_weights_higher_order=w.clone(),
                bipartite_edge_index=ei.clone())
    names = ("edge_index", "edge_weights", "edge_index_higher_order", "edge_weights_higher_order", "bipartite_edge_index")
    object.__setattr__(d, "_pp_hints", {"stamp": tuple((d[k], d[k]._version) for k in names), "rows_sorted": True})
    assert _valid_hints(d).get("rows_sorted") is True
    d.edge_index_higher_order[0, 0] = 1                     # in-place edit: version changes
    assert _valid_hints(d) == {}
    object.__setattr__(d, "_pp_hints", {"stamp": tuple((d[k], d[k]._version) for k in names), "rows_sorted": True})
    assert _valid_hints(d).get("rows_sorted") is True
    d.edge_index = torch.tensor([[2, 0], [1, 1]])           # replaced tensor (not row-sorted any more)
    assert _valid_hints(d) == {}


def test_halo_end_is_a_tight_conservative_bound_for_every_delta_dtype():
    """distributed.halo_end (one searchsorted + one read-back): never smaller than the first event the promoted comparison of
    temporal.py:43 rejects, and at most a rounding step of the float type beyond it."""
    import torch
    from pathpyg_amd.distributed import halo_end
    g = torch.Generator().manual_seed(4)
    for span in (50, 10_000, 2 ** 40):
        t = torch.sort(torch.randint(0, span, (3000,), generator=g)).values
        for delta in (0, 7, span // 10, 3.5, torch.tensor(2.25, dtype=torch.float32), torch.tensor(float(span // 7), dtype=torch.float32),
                      torch.tensor(1e3, dtype=torch.float64)):
            for hi in (1, 17, 1500, 2999):
                thr = t[hi - 1] + (delta if isinstance(delta, torch.Tensor) else torch.as_tensor(delta))
                admitted = t.to(torch.result_type(t, thr)) <= thr
                exact = hi + int(admitted[hi:].to(torch.int64).cumprod(0).sum())          # first id >= hi that is not admitted
                got = halo_end(t, hi, delta)
                assert exact <= got <= t.numel()
                if got > exact:          # extra events lie within the float rounding slack of the threshold
                    slack = float(thr.double().abs()) * 2.0 ** -22 + 2.0
                    assert float(t[got - 1]) <= float(thr.double()) + slack
        tf = torch.sort(torch.rand(500, generator=g, dtype=torch.float64)).values
        assert halo_end(tf, 100, 0.1) == 100 + int((tf[100:] <= tf[99] + 0.1).sum())
    assert halo_end(t, 0, 5) == 0 and halo_end(t, t.numel(), 5) == t.numel()


# ------------------------------------------------------------------ deferred layer tensors (round 5: layers that come out of the order-2 builder)
def test_data_lazy_tensors_resolve_on_first_read_and_answer_sizes_before():
    from pathpyg_amd.data import Data, Lazy
    made = []

    def make():
        made.append(1)
        return torch.arange(6).reshape(2, 3)

    lazy = Lazy(make, (2, 3))
    d = Data(edge_index=lazy, num_nodes=4, edge_weight=torch.ones(3))
    assert d.num_edges == 3 and d.num_nodes == 4 and not made                       # sizes come from the declared shape
    assert d.is_edge_attr("edge_weight") and "edge_index" in d and d.peek("edge_index") is lazy and not made
    assert "edge_index=[2, 3]" in repr(d) and not made
    ei = d.edge_index
    assert made == [1] and torch.equal(ei, torch.arange(6).reshape(2, 3))
    assert d.edge_index is ei and d["edge_index"] is ei and made == [1]               # made once; the bag now holds the tensor itself
    assert d.peek("edge_index") is ei and lazy.value is ei and lazy.version == ei._version
    # clone / to keep what is still deferred deferred (a bundle moved to its device must not materialise every [2, A2] index); iteration and
    # pickling resolve it
    import pickle
    calls = []

    def make5():
        calls.append(1)
        return torch.zeros(2, 5, dtype=torch.long)

    d2 = Data(edge_index=Lazy(make5, (2, 5)), num_nodes=3)
    c = d2.clone().to("cpu")
    assert isinstance(c.peek("edge_index"), Lazy) and c.num_edges == 5 and not calls
    assert c.edge_index.shape == (2, 5) and calls == [1] and isinstance(d2.peek("edge_index"), Lazy)
    assert d2.edge_index is not c.edge_index and calls == [1]                         # (made once: the clone copied the original's tensor)
    back = pickle.loads(pickle.dumps(Data(edge_index=Lazy(make5, (2, 5)), num_nodes=3)))
    assert torch.equal(back.edge_index, torch.zeros(2, 5, dtype=torch.long)) and back.num_nodes == 3
    assert dict(iter(Data(a=Lazy(lambda: torch.ones(2), (2,)))))["a"].shape == (2,)


def test_graph_from_parts_reads_nothing_and_index_map_defers_too():
    import numpy as np
    from pathpyg_amd.core.graph import Graph
    from pathpyg_amd.core.index_map import IndexMap
    from pathpyg_amd.data import Data, Lazy
    made = []

    def deferred(value, name):
        def make():
            made.append(name)
            return value
        return Lazy(make, value.shape)

    ei = torch.tensor([[0, 0, 1], [1, 2, 2]])
    ns = torch.tensor([[0, 1], [0, 2], [1, 2]])
    data = Data(edge_index=deferred(ei, "edge_index"), num_nodes=3, node_sequence=deferred(ns, "node_sequence"), edge_weight=torch.ones(3))
    base = IndexMap(["a", "b", "c"])
    g = Graph._from_parts(data, IndexMap.from_node_sequence(base, data.peek("node_sequence")))
    assert (g.n, g.m, g.order) == (3, 3, 2) and not made                               # sizes and order without touching a tensor
    assert [tuple(r) for r in np.asarray(g.mapping.node_ids).tolist()] == [("a", "b"), ("a", "c"), ("b", "c")] and made == ["node_sequence"]
    assert torch.equal(g.data.edge_index, ei) and made == ["node_sequence", "edge_index"]
    assert torch.equal(g.data.node_sequence, ns) and made == ["node_sequence", "edge_index"]     # (the map's read and the bag's read share one tensor)


def test_dbgnn_forward_honours_handed_plans_only_while_the_bundle_is_untouched():
    from types import SimpleNamespace

    from pathpyg_amd.data import Data, Lazy
    from pathpyg_amd.nn.dbgnn import _valid_plans
    names = ("edge_index", "edge_weights", "edge_index_higher_order", "edge_weights_higher_order", "bipartite_edge_index")
    lazies = {n: Lazy(lambda: torch.zeros(2, 4, dtype=torch.long), (2, 4)) for n in names if n != "edge_weights"}
    w = torch.ones(4)
    d = Data(num_nodes=3, num_ho_nodes=4, edge_weights=w, **lazies)
    stamp = {n: d.peek(n) for n in names}
    plans = {"fo": SimpleNamespace(n_dst=3), "ho": SimpleNamespace(n_dst=4), "bi": object(), "stamp": stamp, "versions": {"edge_weights": w._version}}
    object.__setattr__(d, "_pp_plans", plans)
    assert _valid_plans(d) == (plans["fo"], plans["ho"], plans["bi"])
    _ = d.edge_index_higher_order                                                       # reading a deferred tensor keeps the plans
    assert _valid_plans(d) is not None
    d.edge_index_higher_order.add_(1)                                                   # editing it in place does not
    assert _valid_plans(d) is None
    d2 = Data(num_nodes=3, num_ho_nodes=4, edge_weights=w, **{n: Lazy(lambda: torch.zeros(2, 4, dtype=torch.long), (2, 4)) for n in lazies})
    object.__setattr__(d2, "_pp_plans", dict(plans, stamp={n: d2.peek(n) for n in names}))
    assert _valid_plans(d2) is not None
    d2.edge_index = torch.zeros(2, 4, dtype=torch.long)                                 # replacing a tensor does not either
    assert _valid_plans(d2) is None
    d3 = Data(num_nodes=5, num_ho_nodes=4, edge_weights=w, **{n: Lazy(lambda: torch.zeros(2, 4, dtype=torch.long), (2, 4)) for n in lazies})
    object.__setattr__(d3, "_pp_plans", dict(plans, stamp={n: d3.peek(n) for n in names}))
    assert _valid_plans(d3) is None                                                     # the bundle's node count no longer matches the plan
    w.mul_(2)
    assert _valid_plans(d) is None


def test_order2_builder_is_not_chosen_for_contact_shaped_streams():
    """`_hip.debruijn2_wanted` (who builds the order-2 model: host logic of `MultiOrderModel.from_temporal_graph(max_order=2)` and
    `distributed.build_dbgnn_shard`): node by node up to 2048 events per node on average, the generic kernels beyond (VERDICT r5 #4a)."""
    from pathpyg_amd import _hip
    assert _hip.debruijn2_wanted(10**7, 5 * 10**5)              # the headline stream: 20 events per node
    assert _hip.debruijn2_wanted(2 * 10**7, 10**6)              # BASELINE configs[2]'s scale-free generator (one node with 2 * 10^6 in-events)
    assert _hip.debruijn2_wanted(28_561, 126)                   # the size of the reference's documented contact datasets: 227 events per node
    assert not _hip.debruijn2_wanted(2 * 10**6, 96)             # 96 nodes / 2 * 10^6 events: every node a hub on both sides


def test_small_grid_cases_are_exact_in_fp32():
    """Every case of tests/test_gpu_small_grid.py, built here without a GPU: each linear output is a multiple of its common denominator and
    the sum of the magnitudes of its terms times that denominator stays below 2^24 (the generators assert it, thinning their gradients
    where a sum over all rows needs it), so the fp32 kernels must reproduce the float64 values bit for bit."""
    from tests import small_grid_cases as sg
    built = 0
    for case_id, build in sg.all_cases():
        case = build()
        assert 0.0 < case.ratio < 1.0, case_id
        assert all(value.abs().max() > 0 for outputs in case.exact.values() for value, _, _ in outputs.values()), case_id
        built += 1
    assert built > 600


def test_value_cases_are_exact_in_front_of_the_epilogue():
    """Every builder of tests/test_gpu_value_domain.py, run here without a GPU: what stands in front of the ELU / ELU' epilogue, evaluated by
    torch on the CPU in fp32 and in float64, is the same numbers (each sum has one non-zero term: a grid value, times a power of two on the
    gradient side), and every grid value stands in every column.  The cross-entropy reference of the same module (``F.cross_entropy`` on float64
    logits) agrees with the formula written out, its Adam reference with a float64 ``torch.optim.Adam``."""
    import torch.nn.functional as F
    from tests import value_cases as vc
    x, want = vc.ELU_GRID
    assert x.dtype == torch.float32 and want.dtype == torch.float64 and torch.equal(want, torch.where(x > 0, x.double(), torch.expm1(x.double())))
    for lo, hi in ((-0.25, 0.0), (-100.0, -0.25), (0.0, 100.0)):                      # every branch of elu_fast, and the ends of each
        assert bool(((x > lo) & (x < hi)).any()) and bool((x == lo).any()) and bool((x == hi).any())
    assert int((x == 0).sum()) == 2 and bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())
    act = vc.ACT_GRID
    for value in (-1.0, -1.0 + 2.0 ** -24, 0.0, vc.TINY):
        assert bool((act == value).any()), value
    assert bool((act >= -1).all()) and bool(torch.signbit(act[act == 0]).any())
    built = 0
    for case_id, build, everywhere in vc.all_cases():
        case = build()
        f32, f64 = case.front(torch.float32), case.front(torch.float64)
        assert f32.dtype == torch.float32 and torch.equal(f32.double(), f64) and torch.equal(f32, case.pre), case_id
        if everywhere:
            assert vc.covers(getattr(case, "act", case.pre), case.grid), case_id
        built += 1
    assert built > 40
    for kind in vc.CE_KINDS:
        for c in vc.CE_CLASSES:
            z, y = vc.cross_entropy_case(kind, 1000, c)
            (loss, grad), (plain, plain_grad) = vc.cross_entropy_reference(z, y), vc.cross_entropy_plain(z, y)
            assert bool(torch.isinf(loss)) == (kind == "masked_target") and bool(torch.isfinite(grad).all()), (kind, c)
            torch.testing.assert_close(loss, plain, rtol=1e-7 if kind == "margin20" else 1e-11, atol=0.0)
            torch.testing.assert_close(grad, plain_grad, rtol=1e-11, atol=1e-18)
            if kind.startswith("masked"):
                assert bool((grad[torch.isinf(z) & (F.one_hot(y, c) == 0)] == 0).all()), (kind, c)
    init, grads = vc.adam_inputs()
    params = [torch.nn.Parameter(t.double().clone()) for t in init]
    opt = torch.optim.Adam(params, **vc.ADAM)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.double()
        opt.step()
    for p, mine in zip(params, vc.adam_reference(init, grads, **vc.ADAM)):
        torch.testing.assert_close(mine, p.detach(), rtol=1e-12, atol=1e-14)
