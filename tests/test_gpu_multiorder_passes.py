"""GPU tests of the level-by-level builder taking its levels in PASSES over ranges of types (``core/multi_order_passes.py``,
``pp_multiorder_split`` / ``pp_multiorder_concat``): ``MultiOrderModel.from_temporal_graph(max_order >= 3)`` with
``multi_order_model.PASS_INSTANCES`` set to a fraction of a level against the same build with the default budget — layer tensors bit for bit,
arbitrary float32 weights included: the instances of a type stay together, so every merged weight is summed in the same order — and against
the CPU oracle; the two kernels called directly; the default path, which must not enter the new code; the ``inverse_idx`` of a layer with
more instances than the generic kernels number."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_multiorder import _check_against_oracle, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["sparse", "hubs", "contact", "ties", "loops"]
KEYS = ("edge_index", "edge_weight", "node_sequence")
I32 = 0x7ffffff0


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def _prime_at_or_below(x):
    x = max(int(x), 2)
    while any(x % d == 0 for d in range(2, int(x ** 0.5) + 1)):
        x -= 1
    return x


def _graph(pp, kind, weighted):
    if kind == "small":             # about 300 events: what a budget of ONE instance per part is run on
        rng = np.random.default_rng(7)
        m, n, delta = 300, 20, 100
        ei, t = torch.from_numpy(rng.integers(0, n, (2, m))), torch.from_numpy(rng.integers(0, 1_500, m))
    else:
        ei, t, _, n, delta = _stream(kind, 11)
    data = pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=n)
    if weighted:                    # arbitrary float32 weights: sums that depend on their order
        data["edge_weight"] = torch.from_numpy(np.random.default_rng(5).random(ei.size(1)).astype(np.float32) * 3 + 0.01).to(DEV)
    return pp.TemporalGraph(data), delta


def _tensors(model):
    return {k: {key: layer.data[key].cpu() for key in KEYS} for k, layer in model.layers.items()}


@functools.lru_cache(maxsize=None)
def _single_pass(kind, weighted, K, cached=True):
    """The build with the default budget: ``(layer tensors on the host, sizes)``, made once per stream."""
    import pathpyg_amd as pp
    g, delta = _graph(pp, kind, weighted)
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=K, cached=cached)
    assert "layers" in getattr(model, "sizes", {}), "the level-by-level builder did not take the stream"
    assert model.sizes["passes"] == [1] * K
    return _tensors(model), model.sizes


def _budget(sizes, which):
    most = max(x[2] for x in sizes["layers"][1:])
    return [-(-most // 3), -(-most // 10), _prime_at_or_below(most // 10), 1][which]


def _in_passes(pp, monkeypatch, kind, weighted, K, which, cached=True):
    from pathpyg_amd.core import multi_order_model as mm
    want, sizes = _single_pass(kind, weighted, K, cached)
    budget = _budget(sizes, which)
    monkeypatch.setattr(mm, "PASS_INSTANCES", budget)
    g, delta = _graph(pp, kind, weighted)
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=K, cached=cached)
    assert "layers" in getattr(model, "sizes", {}), "the build in passes handed the stream back"
    got = _tensors(model)
    assert sorted(got) == sorted(want)
    for k in want:
        for key in KEYS:
            assert got[k][key].dtype == want[k][key].dtype and torch.equal(got[k][key], want[k][key]), (k, key)
    assert model.sizes["layers"] == sizes["layers"]
    passes = model.sizes["passes"]
    assert len(passes) == K and passes[0] == 1 and max(passes) > 1, passes
    # a level of E instances in parts of at most max(budget, largest type) <= budget + 4096: at least E / (budget + 4096) parts
    for k in range(1, K):
        assert passes[k] >= sizes["layers"][k][2] / (budget + 4096), (k, passes)
    return model, budget


@pytest.mark.parametrize("K,which", [(4, 0), (4, 1), (4, 2), (5, 2)])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_passes_equal_the_single_pass_build(pp, monkeypatch, kind, weighted, K, which):
    _in_passes(pp, monkeypatch, kind, weighted, K, which)


def test_top_layer_only(pp, monkeypatch):
    model, _ = _in_passes(pp, monkeypatch, "hubs", True, 5, 1, cached=False)
    assert sorted(model.layers) == [5]


@pytest.mark.parametrize("weighted", [False, True])
def test_one_instance_per_part(pp, monkeypatch, weighted):
    model, budget = _in_passes(pp, monkeypatch, "small", weighted, 4, 3)
    assert budget == 1
    # every type that has children is a part of its own, the childless ones ride along: no fewer parts than types with children
    sizes = model.sizes["layers"]
    for k in range(1, 4):
        with_children = int((torch.bincount(model.layers[k + 1].data.edge_index[0], minlength=sizes[k][0]) > 0).sum())
        assert with_children <= model.sizes["passes"][k] <= sizes[k][0]


@pytest.mark.parametrize("kind,weighted", [("contact", False), ("ties", True), ("loops", False), ("loops", True), ("small", True)])
def test_passes_equal_the_oracle(pp, monkeypatch, kind, weighted):
    from pathpyg_amd.core import multi_order_model as mm
    _, sizes = _single_pass(kind, False, 4)
    monkeypatch.setattr(mm, "PASS_INSTANCES", _budget(sizes, 1))
    if kind == "small":
        g, delta = _graph(pp, kind, False)
        ei, t, n = g.data.edge_index.cpu(), g.data.time.cpu(), int(g.data.num_nodes)
        w = torch.from_numpy(np.random.default_rng(2).integers(1, 4, ei.size(1)).astype(np.float32))
    else:
        ei, t, w, n, delta = _stream(kind, 11)
    model = _check_against_oracle(pp, ei, t, w, n, delta, 4, True, weighted)          # (layer tensors AND inverse_idx)
    assert max(model.sizes["passes"]) > 1


def test_default_build_never_enters_the_new_code(pp, monkeypatch):
    from pathpyg_amd import _hip
    from pathpyg_amd.core import multi_order_passes

    def boom(*a, **kw):
        raise AssertionError("the default path called into the passes")
    monkeypatch.setattr(_hip, "multi_order_split", boom)
    monkeypatch.setattr(_hip, "multi_order_concat", boom)
    monkeypatch.setattr(multi_order_passes, "continue_in_passes", boom)
    g, delta = _graph(pp, "hubs", True)
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=4)
    assert "layers" in model.sizes and model.sizes["passes"] == [1, 1, 1, 1]
    assert all(isinstance(x[2], int) for x in model.sizes["layers"])


def test_inverse_idx_names_the_limit(pp, monkeypatch):
    from pathpyg_amd.core import multi_order_model as mm
    from pathpyg_amd.data import Lazy
    want, sizes = _single_pass("loops", False, 4)
    e = [x[2] for x in sizes["layers"]]                       # instances of the orders 1 .. 4
    g, delta = _graph(pp, "loops", False)
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=4)
    assert e[0] < e[1] < e[2] < e[3], "the stream was chosen for instance counts that grow with the order"
    limit = e[3]                                              # as if order 4 were the first with more instances than the generic kernels number
    monkeypatch.setattr(mm, "_INT32_ROWS", limit)
    model.to(DEV)                                             # moving keeps the value deferred: nothing is built, nothing raises
    assert isinstance(model.layers[4].data.peek("inverse_idx"), Lazy)
    with pytest.raises(RuntimeError, match=rf"layer 4 has {e[3]} instances.*fewer than {limit}"):
        model.layers[4].data.inverse_idx
    # the shared generic build stops at order 3: that layer's inverse_idx is still served, and equals the unlimited build's
    monkeypatch.setattr(mm.MultiOrderModel, "_from_temporal_graph_generic", staticmethod(_only_up_to(3, mm.MultiOrderModel._from_temporal_graph_generic)))
    got = model.layers[3].data.inverse_idx.cpu()
    monkeypatch.undo()
    full = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=4)
    assert torch.equal(got, full.layers[3].data.inverse_idx.cpu())


def _only_up_to(order, generic):
    def checked(g, delta, max_order, *rest):
        assert max_order == order, f"the generic build was asked for order {max_order}, not {order}"
        return generic(g, delta, max_order, *rest)
    return checked


# ---------------------------------------------------------------------------------------------------------------- the kernels, directly
def _level(counts, parents, dev=DEV):
    """A level with the given per-type child and instance counts; ``ibase`` as the device scan leaves it: the low 32 bits of the prefix."""
    from pathpyg_amd._hip import MultiOrderLevel
    counts, parents = np.asarray(counts, dtype=np.int64), np.asarray(parents, dtype=np.int64)
    prefix = np.concatenate(([0], np.cumsum(counts)))
    ibase = torch.from_numpy((prefix & 0xffffffff).astype(np.uint32).view(np.int32).copy()).to(dev)
    tptr_host = np.concatenate(([0], np.cumsum(parents)))
    t, n_inst = counts.size, int(tptr_host[-1])
    ids = torch.arange(t, dtype=torch.int32, device=dev)
    inst = torch.arange(4 * n_inst, dtype=torch.int32, device=dev).view(n_inst, 4)
    level = MultiOrderLevel(types=t, children=int(prefix[-1]), status=0, tptr=torch.from_numpy(tptr_host.astype(np.int32)).to(dev), ibase=ibase,
                            inst=inst, row_ptr=None, col=ids + 100, weight=ids.float(), tlast=ids + 7)
    return level, prefix, tptr_host


def _check_split(level, prefix, tptr_host, budget):
    from pathpyg_amd import _hip
    from pathpyg_amd.core.multi_order_passes import greedy_cuts
    parts = _hip.multi_order_split(level, budget)
    cuts = greedy_cuts(prefix.tolist(), budget)
    assert [0] + list(np.cumsum([p.types for p in parts])) == cuts
    for p, (a, b) in zip(parts, zip(cuts, cuts[1:])):
        assert p.children == int(prefix[b] - prefix[a])
        assert p.ibase.dtype == torch.int32 and p.ibase.cpu().tolist() == (prefix[a: b + 1] - prefix[a]).tolist()
        assert p.tptr.dtype == torch.int32 and p.tptr.cpu().tolist() == (tptr_host[a: b + 1] - tptr_host[a]).tolist()
        assert torch.equal(p.col, level.col[a:b]) and torch.equal(p.tlast, level.tlast[a:b]) and torch.equal(p.weight, level.weight[a:b])
        assert torch.equal(p.inst, level.inst[int(tptr_host[a]): int(tptr_host[b])])
        assert p.inst.numel() == 0 or p.inst.data_ptr() == level.inst[int(tptr_host[a]):].data_ptr(), "a part's instances are a view"
    return cuts


WRAP_COUNTS = [(1 << 30) - 3, (1 << 30) + 5, 7, 1 << 30, (1 << 30) - 1, 0, (1 << 30) + 11]


@pytest.mark.parametrize("budget,cuts", [(I32 - 1, [0, 1, 3, 4, 6, 7]), (1 << 30, [0, 1, 2, 3, 4, 6, 7])])
def test_split_counts_in_64_bits_behind_a_wrapped_prefix(pp, budget, cuts):
    level, prefix, tptr_host = _level(WRAP_COUNTS, [1, 2, 1, 3, 1, 1, 2])
    assert level.children > 1 << 32 and bool((level.ibase[1:] < level.ibase[:-1]).any()), "the prefix was meant to wrap"
    assert _check_split(level, prefix, tptr_host, budget) == cuts


def test_split_refuses_a_type_no_step_takes(pp):
    from pathpyg_amd import _hip
    level, _, _ = _level([5, 0x7fffffff, 3], [1, 1, 1])
    assert _hip.multi_order_split(level, 1 << 30) is None


def _split_status(tptr, ibase, budget, max_parts):
    """pp_multiorder_split called directly: ``(parts, status)`` of its report, and the rebased arrays as they were left (pre-filled with -1)."""
    from pathpyg_amd._hip import _stream
    from pathpyg_amd._lib import check, lib
    types = len(tptr) - 1
    i32 = dict(dtype=torch.int32, device=DEV)
    tp, ib = torch.tensor(tptr, **i32), torch.tensor(ibase, **i32)
    report = torch.zeros(4 + 3 * (max_parts + 1), dtype=torch.int64, device=DEV)
    tptr_out, ibase_out = torch.full((types + max_parts,), -1, **i32), torch.full((types + max_parts,), -1, **i32)
    ws = torch.empty(max(int(lib().pp_multiorder_split_ws_bytes(types)), 16), dtype=torch.uint8, device=DEV)
    check(lib().pp_multiorder_split(types, tp.data_ptr(), ib.data_ptr(), budget, max_parts, report.data_ptr(), tptr_out.data_ptr(), ibase_out.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()), "pp_multiorder_split")
    host = report.tolist()
    return host[0], host[1], tptr_out.cpu().tolist(), ibase_out.cpu().tolist()


def test_split_reports_a_prefix_that_does_not_ascend(pp):
    # 3 - 5 as an unsigned difference is no count below 2^31: status bit 2, nothing is rebased
    from pathpyg_amd import _hip
    from pathpyg_amd._lib import HipError
    _, status, tptr_out, ibase_out = _split_status([0, 1, 2, 3], [0, 5, 3, 9], 4, 3)
    assert status & 4 and set(tptr_out) == {-1} and set(ibase_out) == {-1}
    level, _, _ = _level([5, 1, 6], [1, 1, 1])
    level.ibase = torch.tensor([0, 5, 3, 9], dtype=torch.int32, device=DEV)
    level.children = 9
    with pytest.raises(HipError, match="status 4"):
        _hip.multi_order_split(level, 4)


def test_split_reports_more_parts_than_there_is_room_for(pp, monkeypatch):
    from pathpyg_amd import _hip
    parts, status, tptr_out, ibase_out = _split_status([0, 1, 2, 3], [0, 3, 6, 9], 3, 1)          # three parts of one type each, room for one
    assert status & 1 and parts == 1 and set(tptr_out) == {-1} and set(ibase_out) == {-1}
    parts, status, tptr_out, ibase_out = _split_status([0, 1, 2, 3], [0, 3, 6, 9], 3, 3)
    assert (parts, status) == (3, 0) and tptr_out == [0, 1, 0, 1, 0, 1] and ibase_out == [0, 3, 0, 3, 0, 3]
    # the wrapper refuses a budget that may need more parts than one split makes, before any launch
    monkeypatch.setattr(_hip, "SPLIT_MAX_PARTS", 2)
    level, _, _ = _level([3, 3, 3], [1, 1, 1])
    with pytest.raises(ValueError, match="at most 2"):
        _hip.multi_order_split(level, 3)
    with pytest.raises(ValueError):                                    # (the library's own bound on max_parts)
        _split_status([0, 1], [0, 3], 3, 2)


@pytest.mark.parametrize("types,budget", [(1, 5), (2, 1), (7, 10), (300, 1), (5_000, 997), (5_000, 10 ** 9), (70_000, 40_000)])
def test_split_cuts_equal_the_host_rule(pp, types, budget):
    rng = np.random.default_rng(types + budget)
    counts = rng.integers(0, 60, types) * (rng.random(types) < 0.7)         # childless types between the others
    parents = rng.integers(1, 4, types)
    level, prefix, tptr_host = _level(counts, parents)
    cuts = _check_split(level, prefix, tptr_host, budget)
    if budget == 1:
        assert len(cuts) - 1 >= int((counts > 0).sum())                     # one type with children per piece
    if budget == 10 ** 9:
        assert cuts == [0, types]


def _pieces(rows_edges, want_last, seed):
    from pathpyg_amd._hip import MultiOrderLevel
    rng = np.random.default_rng(seed)
    pieces, ref_rows, ref = [], [], {"col": [], "weight": [], "last": []}
    at = 0
    for rows, edges in rows_edges:
        if edges is None:                                                   # a part without children
            pieces.append((rows, None))
            ref_rows.append(np.full(rows, at, dtype=np.int64))
            continue
        marks = np.sort(rng.integers(0, edges + 1, rows - 1)) if rows > 1 else np.zeros(0, dtype=np.int64)
        row_ptr = np.concatenate(([0], marks, [edges])).astype(np.int32)
        cap = edges + int(rng.integers(0, 5))                               # (a step's arrays have room for more than its types)
        col, last = rng.integers(0, 1 << 30, cap).astype(np.int32), rng.integers(0, 1 << 20, cap).astype(np.int32)
        weight = rng.random(cap).astype(np.float32)
        pieces.append((rows, MultiOrderLevel(types=edges, children=0, status=0, row_ptr=torch.from_numpy(row_ptr).to(DEV), col=torch.from_numpy(col).to(DEV),
                                             weight=torch.from_numpy(weight).to(DEV), tlast=torch.from_numpy(last).to(DEV) if want_last else None)))
        ref_rows.append(row_ptr[:rows].astype(np.int64) + at)
        for key, a in (("col", col), ("weight", weight), ("last", last)):
            ref[key].append(a[:edges])
        at += edges
    ref_ptr = np.concatenate(ref_rows + [np.array([at])]).astype(np.int32)
    return pieces, ref_ptr, {k: np.concatenate(v) for k, v in ref.items()}


CONCAT = {
    "one": [(5, 9)],
    "two": [(300, 1_000), (1, 3)],
    "seven": [(3, 4), (1, 1), (700, 70_001), (2, 0), (1, 5), (40, 39), (9, 2_049)],
    "empty first": [(4, None), (6, 10), (2, 3)],
    "empty in the middle": [(6, 10), (1, None), (300, None), (2, 3)],
    "empty last": [(6, 10), (2, 3), (5, None)],
    "one type per piece": [(1, e) for e in (3, 1, 0, 8, 2, 1, 1, 5, 4)],
    "more pieces than one launch takes": [(1 + i % 3, (7 * i) % 11) for i in range(75)],
}


@pytest.mark.parametrize("want_last", [True, False])
@pytest.mark.parametrize("name", list(CONCAT))
def test_concat_equals_the_pieces_one_after_another(pp, name, want_last):
    from pathpyg_amd import _hip
    pieces, ref_ptr, ref = _pieces(CONCAT[name], want_last, len(name))
    row_ptr, col, weight, last = _hip.multi_order_concat(pieces, want_last)
    assert row_ptr.dtype == torch.int32 and row_ptr.cpu().numpy().tolist() == ref_ptr.tolist()
    assert col.dtype == torch.int32 and np.array_equal(col.cpu().numpy(), ref["col"])
    assert weight.dtype == torch.float32 and np.array_equal(weight.cpu().numpy(), ref["weight"])
    assert (last is None) == (not want_last)
    if want_last:
        assert last.dtype == torch.int32 and np.array_equal(last.cpu().numpy(), ref["last"])


def test_concat_refuses_a_layer_int32_ids_do_not_hold(pp):
    import ctypes
    from pathpyg_amd._lib import check, lib
    from pathpyg_amd._lib import HipError
    one = torch.zeros(4, dtype=torch.int32, device=DEV)
    ptrs, sizes = ctypes.c_void_p * 2, ctypes.c_int64 * 2
    table = ptrs(one.data_ptr(), one.data_ptr())
    with pytest.raises((HipError, ValueError)):                 # sizes are checked on the host before anything is launched
        check(lib().pp_multiorder_concat(2, table, table, table, None, sizes(1, 1), sizes(1 << 30, 1 << 30), one.data_ptr(), one.data_ptr(),
                                         one.data_ptr(), None, None), "pp_multiorder_concat")
