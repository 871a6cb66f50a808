"""The De Bruijn layers 1..K on N ranks, split by first node (``distributed.build_multi_order_shard`` / ``gather_multi_order``): the PROTOCOL —
cuts, rebasing of the row pointers, empty ranks, the agreement on fallbacks — with the torch / numpy stand-in of the device contracts
(``tests/cpu_ops_multiorder.py``), ranks as threads (``ThreadWorld``) and as ``gloo`` processes, against the CPU oracle, bit for bit.
The kernels themselves are checked on the GPU (``tests/test_gpu_multiorder_sharded.py``)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

KINDS = ["sparse", "hubs", "contact", "ties", "loops", "longlist"]
K = 4
KEYS = ("edge_index", "edge_weight", "node_sequence")


def raw_stream(kind):
    """``(edge_index, time, n, delta)`` as numpy-made tensors, NOT yet sorted by time."""
    if kind == "longlist":          # node 0 has 6008 out-events: beyond the 4096 of the LDS list sort, and 24 % of the level-2 instances
        rng = np.random.default_rng(11)
        m, n, span, delta = 26_000, 3_000, 100_000, 8_000
        ei = rng.integers(0, n, (2, m))
        ei[0, :6000] = 0
        t = rng.integers(0, span, m)
        return torch.from_numpy(ei), torch.from_numpy(t), n, delta
    from tests.test_gpu_multiorder import _stream
    ei, t, _, n, delta = _stream(kind, 11)
    return ei, t, n, delta


def weights_of(mode, m):
    if mode == "unit":
        return None
    if mode == "dyadic":            # sums of these are exact in float32: equality cannot depend on the order a long run is summed in
        return torch.from_numpy((np.random.default_rng(11).integers(1, 32, m) / 8).astype(np.float32))
    return torch.from_numpy(np.random.default_rng(11).random(m).astype(np.float32))


def fake_graph(ei, t, n, w=None):
    """What the drivers read of a TemporalGraph: ``data`` (time-sorted) and ``mapping``."""
    import pathpyg_amd as pp
    from pathpyg_amd.core.index_map import IndexMap
    g = type("G", (), {})()
    g.data = pp.Data(edge_index=ei, time=t, num_nodes=n)
    if w is not None:
        g.data["edge_weight"] = w
    g.mapping = IndexMap()
    return g


@functools.lru_cache(maxsize=None)
def case(kind, mode, max_order=K):
    """``(fake graph on the host, delta, oracle layers)`` of a test stream."""
    from oracle import model as om
    ei, t, n, delta = raw_stream(kind)
    w = weights_of(mode, ei.size(1))
    sei, st, perm = om.stable_time_sort(ei, t)
    sw = None if w is None else w[perm]
    want = om.layers_from_temporal(sei, st, n, delta=delta, max_order=max_order, edge_weight=sw)
    return fake_graph(sei, st, n, sw), delta, want


def _ops():
    from tests.cpu_ops_multiorder import CpuOpsMultiOrder
    return CpuOpsMultiOrder()


def check_model(model, want, inverse_up_to=2):
    assert sorted(model.layers) == sorted(want)
    for k in want:
        d = model.layers[k].data
        for key in KEYS + (("inverse_idx",) if k <= inverse_up_to else ()):
            assert torch.equal(d[key].cpu(), want[k][key]), (k, key)
        assert d.num_nodes == want[k]["num_nodes"]
    assert [x[:2] for x in model.sizes["layers"]] == [(want[k]["num_nodes"], want[k]["edge_index"].size(1)) for k in sorted(want)]


def summary(shard):
    return {"rank": shard.rank, "cuts": shard.cuts,
            "layers": [dict(n_nodes=e.n_nodes, n_edges=e.n_edges, row_lo=e.row_lo, row_hi=e.row_hi, edge_lo=e.edge_lo, n_instances=e.n_instances,
                            owned=int(e.col.numel()), rows=int(e.row_ptr.numel()) - 1, has_last=e.last is not None) for e in shard.layers]}


def check_invariants(parts, want, m, unit):
    """Shard invariants WITHOUT gathering: the ranks' rows tile every layer in rank order, the edge offsets chain, every owned row starts
    with a node of the rank's cut, and no instance is processed twice."""
    world = len(parts)
    cuts = parts[0]["cuts"]
    assert all(p["cuts"] == cuts and p["rank"] == r for r, p in enumerate(parts))
    for k in sorted(want):
        layer = [p["layers"][k - 1] for p in parts]
        n_nodes, n_edges = want[k]["num_nodes"], want[k]["edge_index"].size(1)
        assert all(e["n_nodes"] == n_nodes and e["n_edges"] == n_edges for e in layer), k
        assert layer[0]["row_lo"] == 0 and layer[-1]["row_hi"] == n_nodes and layer[0]["edge_lo"] == 0
        for r in range(world):
            e = layer[r]
            assert e["rows"] == e["row_hi"] - e["row_lo"] >= 0
            assert e["has_last"] == (k < max(want))
            if r + 1 < world:
                assert layer[r + 1]["row_lo"] == e["row_hi"] and layer[r + 1]["edge_lo"] == e["edge_lo"] + e["owned"], (k, r)
            else:
                assert e["edge_lo"] + e["owned"] == n_edges
            first = want[k]["node_sequence"][e["row_lo"]: e["row_hi"], 0]
            assert bool(((first >= cuts[r]) & (first < cuts[r + 1])).all()), (k, r)
        if unit:
            expected = m if k == 1 else int(want[k]["edge_weight"].double().sum())
            assert sum(e["n_instances"] for e in layer) == expected, (k, [e["n_instances"] for e in layer], expected)


def rank_body(comm, kind, mode, max_order=K):
    from pathpyg_amd import distributed as pd
    g, delta, want = case(kind, mode, max_order)
    ops = _ops()
    shard = pd.build_multi_order_shard(g, delta, max_order, comm, ops=ops)
    assert shard is not None, f"{kind}: the level-by-level route refused a stream it must take"
    assert shard.rank == comm.rank and shard.world == comm.world and len(shard.layers) == max_order
    check_model(pd.gather_multi_order(shard, comm, g, ops=ops), want)
    return summary(shard)


# ---------------------------------------------------------------------------------------------------------------- 1. the cuts
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_cuts_are_monotone_and_balanced(world):
    from pathpyg_amd.distributed import multi_order_cuts
    prefixes = []
    for kind in KINDS:
        g, delta, _ = case(kind, "unit")
        _, loads = _ops().multi_order_node_loads(g.data.edge_index, g.data.time, int(g.data.num_nodes), delta)
        assert loads[0][-1] == g.data.edge_index.size(1)
        prefixes.append(loads[1])
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 1000):
        prefixes.append(torch.from_numpy(np.concatenate(([0], np.cumsum(rng.integers(0, 50, n) * (rng.random(n) < 0.3))))))
        prefixes.append(torch.from_numpy(np.concatenate(([0], np.cumsum(rng.integers(0, 1 << 40, n))))))
    prefixes.append(torch.zeros(6, dtype=torch.int64))
    for prefix in prefixes:
        n = prefix.numel() - 1
        cuts = multi_order_cuts(prefix, world)
        assert len(cuts) == world + 1 and cuts[0] == 0 and cuts[-1] == n
        assert all(a <= b for a, b in zip(cuts, cuts[1:]))
        total, most = int(prefix[-1]), int((prefix[1:] - prefix[:-1]).max()) if n else 0
        for r in range(world):
            # what the prefix rule guarantees: a rank stops at the first node that reaches its target
            assert (int(prefix[cuts[r + 1]]) - int(prefix[cuts[r]])) * world <= total + most * world


def test_longlist_is_the_stream_the_issue_describes():
    g, delta, want = case("longlist", "unit")
    assert int((g.data.edge_index[0] == 0).sum()) == 6008
    assert [want[k]["edge_index"].size(1) for k in (1, 2, 3, 4)] == [22_559, 16_133, 11_106, 8_924]


# ---------------------------------------------------------------------------------------------------------------- 2. + 3. ranks as threads
@pytest.mark.parametrize("mode", ["unit", "dyadic"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_thread_world_equals_the_oracle(world, kind, mode):
    from pathpyg_amd.distributed import run_thread_world
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1) // world))
    g, _, want = case(kind, mode)
    parts = run_thread_world(world, lambda comm: rank_body(comm, kind, mode))
    check_invariants(parts, want, g.data.edge_index.size(1), mode == "unit")


# ---------------------------------------------------------------------------------------------------------------- 4. empty ranks
def three_node_case():
    from oracle import model as om
    ei = torch.tensor([[0, 1, 2, 0, 1], [1, 2, 0, 1, 2]])
    t = torch.tensor([1, 2, 3, 4, 5])
    return fake_graph(ei, t, 3), 2, om.layers_from_temporal(ei, t, 3, delta=2, max_order=3)


def test_more_ranks_than_first_nodes():
    from pathpyg_amd import distributed as pd
    g, delta, want = three_node_case()
    assert [(want[k]["num_nodes"], want[k]["edge_index"].size(1)) for k in (1, 2, 3)] == [(3, 3)] * 3

    def body(comm):
        ops = _ops()
        shard = pd.build_multi_order_shard(g, delta, 3, comm, ops=ops)
        assert shard is not None
        check_model(pd.gather_multi_order(shard, comm, g, ops=ops), want)
        return summary(shard)

    parts = pd.run_thread_world(8, body)
    check_invariants(parts, want, 5, True)
    assert sum(1 for p in parts if all(e["owned"] == 0 and e["rows"] == 0 for e in p["layers"])) >= 5
    # the 12 nodes of `contact` on 8 ranks
    g, _, want = case("contact", "unit")
    parts = pd.run_thread_world(8, lambda comm: rank_body(comm, "contact", "unit"))
    check_invariants(parts, want, g.data.edge_index.size(1), True)


# ---------------------------------------------------------------------------------------------------------------- 5. agreement on fallbacks
def fallback_streams():
    """Streams every rank must hand back (``None``) at the same level."""
    from oracle import model as om
    rng = np.random.default_rng(3)
    m, n = 1_500, 2
    ei = torch.from_numpy(rng.integers(0, n, (2, m)))
    t = torch.from_numpy(rng.integers(0, 600, m))
    sei, st, _ = om.stable_time_sort(ei, t)
    many_children = (fake_graph(sei, st, n), 60, 3)              # a layer-2 node with 29 167 continuations
    no_edges = (fake_graph(torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.tensor([1, 5, 10]), 4), 4, 3)      # layer 3: one node, no edge
    return {"many_children": many_children, "no_edges": no_edges}


def fallback_body(comm, which):
    from pathpyg_amd import distributed as pd
    g, delta, max_order = fallback_streams()[which]
    return pd.build_multi_order_shard(g, delta, max_order, comm, ops=_ops()) is None


@pytest.mark.parametrize("which", ["many_children", "no_edges"])
@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_falls_back_threads(world, which):
    from pathpyg_amd.distributed import run_thread_world
    assert run_thread_world(world, lambda comm: fallback_body(comm, which)) == [True] * world


def test_streams_refused_before_any_collective():
    from pathpyg_amd import distributed as pd
    ei, t = torch.tensor([[0, 1, 2], [1, 2, 0]]), torch.tensor([3, 2, 1])
    comm = pd.Comm()
    assert pd.build_multi_order_shard(fake_graph(ei, t, 3), 2, 3, comm, ops=_ops()) is None                     # not sorted by time
    assert pd.build_multi_order_shard(fake_graph(ei, t.flip(0), 3, torch.ones(3, dtype=torch.float64)), 2, 3, comm, ops=_ops()) is None
    assert comm.events == []
    if not torch.cuda.is_available():         # HipOps refuses host tensors itself (the stand-in is given them)
        from pathpyg_amd.nn.sharded import HipOps
        assert HipOps.multi_order_node_loads(ei, t.flip(0), 3, 2) is None


# ---------------------------------------------------------------------------------------------------------------- gloo processes
def _gloo_worker(rank, world, port, results, what):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(max(1, 16 // world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pathpyg_amd import distributed as pd
        comm = pd.Comm()
        assert comm.world == world and comm.rank == rank
        if what == "fallback":
            assert all(fallback_body(comm, which) for which in ("many_children", "no_edges"))
        else:
            for kind in KINDS:
                for mode in ("unit", "dyadic"):
                    g, _, want = case(kind, mode)
                    mine = rank_body(comm, kind, mode)
                    parts = [None] * world
                    dist.all_gather_object(parts, mine)
                    check_invariants(parts, want, g.data.edge_index.size(1), mode == "unit")
            assert comm.sent_bytes["all_gather"] > 0
        results[rank] = "ok"
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_equals_the_oracle(world):
    # all six streams, unit and dyadic weights, in one set of processes per world size
    from tests.test_distributed_cpu import _spawn
    _spawn(_gloo_worker, world, "streams")


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_falls_back_gloo(world):
    from tests.test_distributed_cpu import _spawn
    _spawn(_gloo_worker, world, "fallback")
