"""GPU tests of the De Bruijn layers 1..K on N ranks, split by first node (``pp_multiorder_node_loads`` / ``_prepare_range`` / ``_stitch`` with
the unchanged ``pp_multiorder_step``; ``distributed.build_multi_order_shard`` / ``gather_multi_order``): ranks as threads sharing ``cuda:0``
(RCCL refuses two ranks on one device), against the CPU oracle and against the single-GPU ``MultiOrderModel.from_temporal_graph``, bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_multiorder_sharded_cpu import KINDS, check_invariants, fallback_streams, raw_stream, summary, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 4
ALL_KEYS = ("edge_index", "edge_weight", "node_sequence", "inverse_idx")


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def _graph(pp, ei, t, n, w=None):
    data = pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=n)
    if w is not None:
        data["edge_weight"] = w.to(DEV)
    return pp.TemporalGraph(data)


@functools.lru_cache(maxsize=None)
def _case(kind, mode, max_order=K, cached=True, float_time=False):
    """``(graph on the GPU, delta, oracle layers or None, single-GPU model)``; the oracle is not the yardstick for arbitrary weights."""
    import pathpyg_amd as pp
    from oracle import model as om
    ei, t, n, delta = raw_stream(kind)
    if float_time:
        t, delta = t.double() / 4, delta / 4
    w = weights_of(mode, ei.size(1))
    g = _graph(pp, ei, t, n, w)
    want = None
    if mode != "random":
        sei, st, perm = om.stable_time_sort(ei, t)
        want = om.layers_from_temporal(sei, st, n, delta=delta, max_order=max_order, edge_weight=None if w is None else w[perm], cached=cached)
    single = pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=max_order, cached=cached)
    assert "layers" in getattr(single, "sizes", {}), f"{kind}: the single-GPU build left the level-by-level builder"
    return g, delta, want, single


def _sharded(world, g, delta, max_order, cached=True):
    from pathpyg_amd import distributed as pd

    def body(comm):
        shard = pd.build_multi_order_shard(g, delta, max_order, comm)
        assert shard is not None, "the level-by-level route refused a stream it must take"
        return shard, pd.gather_multi_order(shard, comm, g, cached=cached)

    return pd.run_thread_world(world, body, device=DEV)


def _check(world, kind, mode, max_order=K, cached=True, float_time=False):
    g, delta, want, single = _case(kind, mode, max_order, cached, float_time)
    out = _sharded(world, g, delta, max_order, cached)
    for rank, (shard, model) in enumerate(out):
        assert model.sizes["layers"] == single.sizes["layers"], rank
        assert sorted(model.layers) == sorted(single.layers) == (list(range(1, max_order + 1)) if cached else [max_order])
        for k in model.layers:
            d, s = model.layers[k].data, single.layers[k].data
            assert d.num_nodes == s.num_nodes
            for key in ALL_KEYS:
                if key == "inverse_idx" and k >= 3 and rank > 0:
                    continue            # (one generic build per model: the inverse maps of the layers from 3 on are checked on rank 0)
                assert torch.equal(d[key], s[key]), (rank, k, key, "single GPU")
                if want is not None:
                    assert torch.equal(d[key].cpu(), want[k][key]), (rank, k, key, "oracle")
    if want is not None and cached:
        check_invariants([summary(shard) for shard, _ in out], want, g.data.edge_index.size(1), mode == "unit")


# 6. the gathered model = the oracle = the single-GPU build, all four tensors of every layer
@pytest.mark.parametrize("mode", ["unit", "dyadic"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_sharded_layers_equal_the_oracle_and_the_single_gpu_build(pp, world, kind, mode):
    _check(world, kind, mode)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_arbitrary_weights_sum_in_the_single_gpu_order(pp, world, kind):
    # a type is never split between ranks: each merged weight is the same sum in the same order on both routes
    g, delta, _, single = _case(kind, "random")
    for rank, (shard, model) in enumerate(_sharded(world, g, delta, K)):
        for k in range(1, K + 1):
            assert torch.equal(model.layers[k].data.edge_weight, single.layers[k].data.edge_weight), (rank, k)
            assert torch.equal(model.layers[k].data.edge_index, single.layers[k].data.edge_index), (rank, k)


def test_top_layer_only_and_float_time(pp):
    _check(3, "hubs", "dyadic", max_order=5, cached=False)
    _check(2, "hubs", "dyadic", max_order=K, float_time=True)


# 7. the range entry point on [0, n) IS pp_multiorder_prepare
@pytest.mark.parametrize("weighted", [False, True])
def test_whole_range_reproduces_the_single_gpu_level_one(pp, weighted):
    from pathpyg_amd import _hip
    from pathpyg_amd._hip import _p, _stream, _workspace, check, lib
    g, delta, _, _ = _case("hubs", "dyadic" if weighted else "unit")
    ei, time, n = g.data.edge_index.contiguous(), g.data.time, int(g.data.num_nodes)
    w = g.data["edge_weight"] if weighted else None
    m = ei.size(1)
    windows, loads = _hip.multi_order_node_loads(ei, time, n, delta, w)
    assert loads[0].tolist() == torch.cat((torch.zeros(1, dtype=torch.int64), torch.bincount(ei[0].cpu(), minlength=n).cumsum(0))).tolist()
    assert int(loads[0][-1]) == m
    level, tab = _hip.multi_order_prepare_range(windows, 0, n, 0, m)
    # the whole-stream entry point, as _hip.multi_order_temporal calls it
    L = lib()
    i32, f32 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float32, device=DEV)
    kind, di, df = _hip.resolve_delta(time.dtype, delta)
    lift_ws = _workspace(L.pp_temporal_ws_bytes(m, n), ei.device)
    check(L.pp_temporal_windows(_p(ei), _p(time), 1, m, n, kind, di, df, _p(lift_ws), lift_ws.numel(), _stream()), "pp_temporal_windows")
    tab0, inst = torch.empty((m, 4), **i32), torch.empty((m, 4), **i32)
    tptr, ibase = torch.empty(m + 1, **i32), torch.empty(m + 1, **i32)
    tlast, wm, row_ptr = torch.empty(m, **i32), torch.empty(m, **f32), torch.empty(n + 1, **i32)
    ws = _workspace(L.pp_multiorder_prepare_ws_bytes(m), ei.device)
    check(L.pp_multiorder_prepare(_p(ei), m, n, _p(w), _p(lift_ws), lift_ws.numel(), 0, _p(tab0), _p(inst), _p(tptr), _p(ibase), _p(tlast), _p(wm),
                                  _p(row_ptr), _p(ws), ws.numel(), _stream()), "pp_multiorder_prepare")
    types, status, children, _ = ws[:32].view(torch.int64).tolist()
    assert (level.types, level.status, level.children) == (types, status, children) and status == 0
    assert int(loads[1][-1]) == children
    assert torch.equal(level.inst, inst) and torch.equal(tab, tab0)
    assert torch.equal(level.tptr[: types + 1], tptr[: types + 1]) and torch.equal(level.ibase[: types + 1], ibase[: types + 1])
    assert torch.equal(level.tlast[:types], tlast[:types]) and torch.equal(level.weight[:types], wm[:types]) and torch.equal(level.row_ptr, row_ptr)
    # and the radix route of the range (forced) gives the same instances in the same order
    ws2 = _workspace(L.pp_multiorder_prepare_range_ws_bytes(m, m), ei.device)
    inst2, tptr2, tlast2 = torch.empty((m, 4), **i32), torch.empty(m + 1, **i32), torch.empty(m, **i32)
    ibase2, w2, row2, tab2 = torch.empty(m + 1, **i32), torch.empty(m, **f32), torch.empty(n + 1, **i32), torch.empty((m, 4), **i32)
    check(L.pp_multiorder_prepare_range(_p(ei), m, n, _p(w), _p(lift_ws), lift_ws.numel(), 0, n, 0, m, 1, _p(tab2), _p(inst2), _p(tptr2), _p(ibase2),
                                        _p(tlast2), _p(w2), _p(row2), _p(ws2), ws2.numel(), _stream()), "pp_multiorder_prepare_range")
    assert ws2[:24].view(torch.int64).tolist() == [types, 0, children]
    assert torch.equal(inst2, inst) and torch.equal(tab2, tab0) and torch.equal(row2, row_ptr)
    assert torch.equal(tptr2[: types + 1], tptr[: types + 1]) and torch.equal(ibase2[: types + 1], ibase[: types + 1])
    assert torch.equal(tlast2[:types], tlast[:types]) and torch.equal(w2[:types], wm[:types])


def test_stitch_rebases_and_concatenates(pp):
    from pathpyg_amd import _hip
    rng = np.random.default_rng(5)
    world, row_lo, edge_lo = 5, [0, 4, 4, 9, 9, 12], [0, 7, 7, 8, 8, 20]
    stride, last_at = 20, 5
    blocks = torch.from_numpy(rng.integers(0, 1000, (world, stride)).astype(np.int32))
    ptr, last = _hip.multi_order_stitch(blocks.reshape(-1).to(DEV), stride, last_at, row_lo, edge_lo)
    want_ptr = [int(blocks[r, i]) + edge_lo[r] for r in range(world) for i in range(row_lo[r + 1] - row_lo[r])] + [20]
    want_last = [int(blocks[r, last_at + i]) for r in range(world) for i in range(edge_lo[r + 1] - edge_lo[r])]
    assert ptr.tolist() == want_ptr and last.tolist() == want_last
    with pytest.raises(ValueError):           # a piece that does not fit its block is refused on the host, nothing is launched
        _hip.multi_order_stitch(blocks.reshape(-1).to(DEV), stride, 3, row_lo, edge_lo)


# 8. agreement on fallbacks with the real kernels
@pytest.mark.parametrize("which", ["many_children", "no_edges"])
@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_falls_back(pp, world, which):
    from pathpyg_amd import distributed as pd
    g_host, delta, max_order = fallback_streams()[which]
    g = _graph(pp, g_host.data.edge_index, g_host.data.time, int(g_host.data.num_nodes))
    assert pd.run_thread_world(world, lambda comm: pd.build_multi_order_shard(g, delta, max_order, comm) is None, device=DEV) == [True] * world
    # host-resident tensors: HipOps refuses them before any collective
    comm = pd.Comm()
    assert pd.build_multi_order_shard(g_host, delta, max_order, comm) is None and comm.events == []


# 9. full size, 8 ranks on one GPU: the two shapes of tests/test_gpu_scale.py::test_multi_order_at_full_size_equals_the_generic_kernels
def _scale_stream(seed, m, n, span, zipf=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    src = torch.randint(0, n, (m,), generator=g, device=DEV)
    if zipf:        # scale-free destinations: heavy hubs
        u = torch.rand(m, generator=g, device=DEV, dtype=torch.float64)
        dst = (n * u.pow(6.0)).long().clamp_(max=n - 1)
    else:
        dst = torch.randint(0, n, (m,), generator=g, device=DEV)
    t = torch.randint(0, span, (m,), generator=g, device=DEV)
    return torch.stack((src, dst)), t


def full_size_body(shape):
    """Runs in a process of its own (one per shape, under a time limit): 8 ranks' shards against the single-GPU MultiOrderLayer arrays."""
    import pathpyg_amd as pp
    from pathpyg_amd import _hip
    from pathpyg_amd import distributed as pd
    if shape == "headline":
        n, m, span, delta, max_order, zipf = 500_000, 10_000_000, 10_000_000, 1_000_000, 5, False
    else:
        n, m, span, delta, max_order, zipf = 1_000_000, 20_000_000, 10_000_000, 1_500_000, 3, True
    ei, t = _scale_stream(3, m, n, span, zipf=zipf)
    g = pp.TemporalGraph(pp.Data(edge_index=ei, time=t, num_nodes=n))
    del ei, t
    single = _hip.multi_order_temporal(g.data.edge_index, g.data.time, n, delta, None, max_order)
    assert single is not None, "the single-GPU build left the level-by-level builder"
    shards = pd.run_thread_world(8, lambda comm: pd.build_multi_order_shard(g, delta, max_order, comm), device=DEV)
    assert all(s is not None for s in shards)
    for k, want in enumerate(single, start=1):
        mine = [s.layers[k - 1] for s in shards]
        assert all((e.n_nodes, e.n_edges) == (want.n_nodes, want.n_edges) for e in mine), k
        assert sum(e.n_instances for e in mine) == want.n_instances, (k, [e.n_instances for e in mine], want.n_instances)
        row_ptr = torch.cat([e.row_ptr[:-1] + e.edge_lo for e in mine] + [torch.tensor([want.n_edges], dtype=torch.int32, device=DEV)])
        assert torch.equal(row_ptr, want.row_ptr), (k, "row_ptr")
        assert torch.equal(torch.cat([e.col for e in mine]), want.col), (k, "col")
        assert torch.equal(torch.cat([e.weight for e in mine]), want.weight), (k, "weight")
        print(f"{shape} layer {k}: {want.n_nodes} nodes, {want.n_edges} edges, instances per rank {[e.n_instances for e in mine]}", flush=True)
        del row_ptr
        for s in shards:
            s.layers[k - 1] = None
        single[k - 1] = None
        torch.cuda.empty_cache()
    print("full size ok", flush=True)


# The time limits.  The existing full-size test (single build + generic build + comparison of every layer tensor) takes 0.9 s (headline, stream
# set-up included) and 0.1 s (configs[2]) inside a warm process; a child process here takes 3.3 s per shape, of which about 2.5 s are the
# interpreter, the imports and the HIP context.  60 s is some twenty times that: a loaded machine does not fail it, a hang still ends.
@pytest.mark.parametrize("shape,limit_s", [("headline", 60), ("scale_free", 60)])
def test_full_size_shards_equal_the_single_gpu_arrays(pp, shape, limit_s):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"from tests.test_gpu_multiorder_sharded import full_size_body; full_size_body({shape!r})"
    done = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=limit_s)
    print(done.stdout[-3000:])
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert "full size ok" in done.stdout
