"""GPU tests of the north-star split (edge-range sharded lift -> destination-owner aggregation -> destination-partitioned DBGNN) with
the REAL HIP kernels:
  * world size 1 (no process group): every collective is the identity — must agree with the oracle and with the single-GPU API path;
  * 2 and 3 ranks SHARING cuda:0 under the gloo backend (collectives staged through the host — test transport only): exercises
    halo exchange, rectangular plans (pp_gcn_plan_begin/_finish), n_self < n_rows in the fused backward kernels on hardware;
  * bench.py end to end through RCCL at world size 1 and through gloo at world size 2.
The GPU box has one GPU, so multi-rank RCCL itself cannot run here; its code path is the same Comm calls with device buffers."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.tolerance import assert_embeddings_close, assert_gradients_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-5, 2e-6


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case(seed, m, n, delta, span, f, hidden, weighted):
    from oracle import dbgnn as od
    from oracle import model as om
    rng = np.random.default_rng(seed)
    ei = torch.from_numpy(rng.integers(0, n, (2, m)))
    t = torch.from_numpy(np.sort(rng.integers(0, span, m)))
    w = torch.from_numpy(rng.integers(1, 4, m).astype(np.float32)) if weighted else None
    layers = om.layers_from_temporal(ei, t, n, delta=delta, max_order=2, edge_weight=w)
    gen = torch.Generator().manual_seed(seed + 1)
    x, x_h = torch.randn(n, f, generator=gen), torch.randn(layers[2]["num_nodes"], f, generator=gen)
    y = torch.randint(0, 3, (n,), generator=gen)
    params = od.init_params(3, (f, f), hidden, seed=seed + 2)
    want = od.loss_and_grads(params, om.dbgnn_inputs(layers, 2, "last", x=x, x_h=x_h), y)
    return ei, t, w, x, x_h, y, params, want, layers


CASES = [
    (3, 6000, 60, 12, 900, 16, [32, 32, 16], True),          # fused <=64-wide kernels
    (4, 9000, 150, 40, 4000, 64, [64, 64, 64], False),       # the benchmark's widths
    (5, 4000, 80, 25, 2000, 128, [128, 128, 64], True),      # 128-wide fused layers (pp_gcn_input_grad_f32 with n_self < n_rows)
    (8, 3000, 70, 20, 1500, 256, [256, 256, 64], False),      # 256-wide layers (weights streamed through LDS) on rectangular plans
    (6, 1500, 40, 9, 500, 8, [12, 10, 6], True),             # widths without a fused kernel: library GEMM + CSR kernels
    (7, 60, 50, 2, 80, 16, [16, 16, 16], False),             # nearly empty higher-order graph, ranks without edges
    (9, 4000, 400, 60, 6000, 64, [64, 64, 64], False),       # ~10 events per node: at world size 1 the fused order-2 builder (pp_debruijn2_*)
    (10, 3000, 350, 45, 5000, 32, [32, 32, 16], True),       # ... with event weights
]


def _lifted_pairs(ei, t, n, delta):
    from oracle import lift as ol
    from oracle import model as om
    sei, st, _ = om.stable_time_sort(ei, t)
    return ol.temporal_lift_sorted(sei, st, delta, n).size(1)


def _run_rank(rank, world, dev, comm, case):
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    ei, t, w, x, x_h, y, params, want, layers = _case(*case)
    want_out, want_loss, want_grads = want
    attrs = {} if w is None else {"edge_weight": w.to(dev)}
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(dev), time=t.to(dev), num_nodes=case[2], **attrs))
    shard = pd.build_dbgnn_shard(tg, case[3], x.to(dev), x_h.to(dev), y.to(dev), comm)
    sz = pd.global_sizes(shard, comm)
    assert sz["U2"] == layers[2]["num_nodes"] and sz["A2"] == layers[2]["edge_index"].size(1)
    if case[0] in (9, 10):          # ~10 events per node: the node-by-node order-2 builder, at every world size (world > 1: node-range partition)
        assert shard.sizes.get("builder") == "fused" and sz["E2"] == int(_lifted_pairs(ei, t, case[2], case[3]))
    if shard.ho.n_send and shard.ho.send_idx is not None:
        assert int(torch.bincount(shard.ho.send_idx).max()) == 1          # De Bruijn cuts: every row goes to at most one peer
    net = pp.nn.DBGNN(num_classes=3, num_features=(case[5], case[5]), hidden_dims=case[6]).to(dev)
    net.load_state_dict(params)
    sharded = pd.ShardedDBGNN(net, comm)
    out = sharded(shard)
    assert_embeddings_close(out, want_out[shard.fo.lo: shard.fo.hi])
    loss = sharded.loss(shard)
    loss.backward()
    pd.all_reduce_gradients(net, average=False, comm=comm)
    total = loss.detach().clone().reshape(1)
    comm.all_reduce_(total)
    torch.testing.assert_close(total.cpu()[0], want_loss, rtol=RTOL, atol=ATOL)
    for name, p in net.named_parameters():
        assert_gradients_close(p.grad, want_grads[name], name)
    return shard, net


@pytest.mark.parametrize("case", CASES, ids=[f"F{c[5]}_m{c[1]}" for c in CASES])
def test_partition_path_world1_matches_oracle_and_api_path(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    dev = torch.device("cuda:0")
    comm = pd.Comm()
    assert comm.world == 1
    shard, net = _run_rank(0, 1, dev, comm, case)
    # the same step through the single-GPU API (MultiOrderModel + DBGNN): identical kernels, identical numbers
    ei, t, w, x, x_h, y, params, want, layers = _case(*case)
    attrs = {} if w is None else {"edge_weight": w.to(dev)}
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(dev), time=t.to(dev), num_nodes=case[2], **attrs))
    mom = pp.MultiOrderModel.from_temporal_graph(tg, delta=case[3], max_order=2)
    data = mom.to_dbgnn_data(max_order=2, x=x.to(dev), x_h=x_h.to(dev))
    net2 = pp.nn.DBGNN(num_classes=3, num_features=(case[5], case[5]), hidden_dims=case[6]).to(dev)
    net2.load_state_dict(params)
    loss2 = pp.nn.cross_entropy(net2(data), y.to(dev))
    loss2.backward()
    for (name, p), (_, q) in zip(net.named_parameters(), net2.named_parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-5, atol=1e-6, msg=lambda s: f"{name}: {s}")


def _gloo_worker(rank, world, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sys.path.insert(0, ROOT)
        from pathpyg_amd import distributed as pd
        torch.cuda.set_device(0)
        dev = torch.device("cuda:0")
        comm = pd.Comm()
        assert comm.world == world and not comm.native
        for case in CASES:
            _run_rank(rank, world, dev, comm, case)
        torch.cuda.synchronize()
        results[rank] = "ok"
    finally:
        dist.destroy_process_group()


def _rccl_worker(rank, world, port, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        sys.path.insert(0, ROOT)
        import pathpyg_amd as pp
        from pathpyg_amd import distributed as pd
        comm = pd.Comm()
        assert comm.world == world and comm.native
        for case in CASES:
            shard, net = _run_rank(rank, world, dev, comm, case)                     # interleaved schedule, native asynchronous collectives
            grads = {k: p.grad.clone() for k, p in net.named_parameters()}
            net.zero_grad(set_to_none=True)
            serial = pd.ShardedDBGNN(net, comm, overlap=False)                       # the same step, every exchange waited for where it is issued
            serial.loss(shard).backward()
            pd.all_reduce_gradients(net, average=False, comm=comm)
            for k, p in net.named_parameters():
                torch.testing.assert_close(p.grad, grads[k], rtol=1e-5, atol=1e-6, msg=lambda s: f"{k} (overlap vs serial): {s}")
        torch.cuda.synchronize()
        results[rank] = "ok"
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL refuses two ranks on one device (the GPU test boxes of this "
                                                          "project have one; the driver's multi-GPU bench is the first place this path runs)")
def test_partition_path_two_ranks_over_rccl_overlap_matches_serial():
    """the native asynchronous collectives (Comm._Pending: all_to_all_single / reduce_scatter_tensor / all_gather_into_tensor with
    async_op=True) and the stream ordering the _ShardedTrunk schedule relies on — against the oracle and against the serial schedule."""
    ctx = mp.get_context("spawn")
    results = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, 2, port, results)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(900)
        assert p.exitcode == 0
    assert dict(results) == {0: "ok", 1: "ok"}


def test_partition_path_three_ranks_as_threads_match_oracle():
    """World size 3 (uneven cuts) with the real kernels, the ranks as threads of this process (ThreadWorld: seconds instead of the minute
    three processes spend switching contexts on one GPU)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from pathpyg_amd import distributed as pd
    dev = torch.device("cuda:0")

    def body(comm):
        for case in CASES:
            _run_rank(comm.rank, 3, dev, comm, case)
        return "ok"

    assert pd.run_thread_world(3, body, dev) == ["ok"] * 3


def test_stream_primitives_eight_ranks_as_threads_match_single_process():
    """The stream primitives on 8 emulated ranks with the real kernels: the concatenated second_order_layer_sharded slices are the
    single-process layer 2, and gather_lifted of every rank's sharded lift block is the whole lift."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd as pp
    from pathpyg_amd import _hip, distributed as pd
    from oracle import model as om
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    m, n, delta = 20_000, 200, 9
    ei = torch.from_numpy(rng.integers(0, n, (2, m)))
    t = torch.from_numpy(np.sort(rng.integers(0, 3000, m)))
    w = torch.from_numpy(rng.integers(1, 4, m).astype(np.float32))
    g = pp.TemporalGraph(pp.Data(edge_index=ei.to(dev), time=t.to(dev), num_nodes=n))
    want = om.layers_from_temporal(ei, t, n, delta=delta, max_order=2, edge_weight=w)[2]
    want_lift = _hip.temporal_lift(ei.to(dev), t.to(dev), n, delta).cpu()
    want_line = _hip.linegraph_lift(want_lift.to(dev), m).cpu()

    def body(comm):
        part = pd.second_order_layer_sharded(g, delta=delta, edge_weight=w.to(dev), comm=comm)
        local, _, total = pd.lift_order_temporal_sharded(g, delta, comm=comm)
        local3, _, total3 = pd.lift_order_edge_index_sharded(want_lift.to(dev), m, comm=comm)
        return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in part.items()} | {
            "lifted": pd.gather_lifted(local, comm=comm).cpu(), "total": total, "line": pd.gather_lifted(local3, comm=comm).cpu(), "total3": total3}

    parts = pd.run_thread_world(8, body, dev)
    for part in parts:
        assert torch.equal(part["node_sequence"], want["node_sequence"]) and part["num_nodes"] == want["num_nodes"]
        assert torch.equal(part["lifted"], want_lift) and part["total"] == want_lift.size(1)
        assert torch.equal(part["line"], want_line) and part["total3"] == want_line.size(1)
    assert torch.equal(torch.cat([p["edge_index"] for p in parts], dim=1), want["edge_index"])
    assert torch.equal(torch.cat([p["edge_weight"] for p in parts]), want["edge_weight"])
    assert torch.equal(torch.cat([p["own_event_ids"] for p in parts]), want["inverse_idx"])


def test_emulation_clocks_events_and_drain_agree_on_results_and_log_every_asynchronous_collective():
    """bench.py --emulate-clock: the "events" clock (turns bracketed by stream events, nothing drained at the collectives; the ranks' data hand-offs
    are ordered by the shared stream alone) must give the results of the "drain" clock, positive device and host times per rank, and one
    (issue, wait) window per asynchronous collective with issue <= wait on the rank's compute clock."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from pathpyg_amd import distributed as pd
    dev = torch.device("cuda:0")
    out = {}
    for clock in ("drain", "events"):
        def body(comm):
            comm.reset_counters()
            shard, net = _run_rank(comm.rank, 4, dev, comm, CASES[0])
            comm.end_turns()
            windows = [(i, comm.position(a), comm.position(b)) for i, a, b in comm.windows]
            n_async = sum(1 for _, _, overlapped in comm.events if overlapped)
            grads = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()
            return comm.compute_s, comm.host_s, windows, n_async, grads
        out[clock] = pd.run_thread_world(4, body, dev, clock=clock)
    for rank in range(4):
        for clock in ("drain", "events"):
            compute_s, host_s, windows, n_async, _ = out[clock][rank]
            assert compute_s > 0 and host_s > 0, (clock, rank)
            assert n_async > 0 and len(windows) == n_async, (clock, rank, len(windows), n_async)
            assert all(0 <= a <= b <= compute_s * 1.001 + 1e-9 for _, a, b in windows), (clock, rank, windows)
        torch.testing.assert_close(out["events"][rank][4], out["drain"][rank][4], rtol=1e-5, atol=1e-7)      # (same kernels; float atomics may reorder)


@pytest.mark.parametrize("world", [2])
def test_partition_path_ranks_sharing_one_gpu_match_oracle(world):
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    ctx = mp.get_context("spawn")
    results = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, results)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    assert dict(results) == {r: "ok" for r in range(world)}


def _zipf_case(seed, m, n, delta, span, f, hidden):
    """Scale-free stream (destinations ~ Zipf(1.2), SURVEY §8d C3 generator), weighted events."""
    from oracle import dbgnn as od
    from oracle import model as om
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n + 1) ** 1.2
    dst = rng.permutation(n)[rng.choice(n, size=m, p=p / p.sum())]
    ei = torch.from_numpy(np.stack((rng.integers(0, n, m), dst)))
    t = torch.from_numpy(np.sort(rng.integers(0, span, m)))
    w = torch.from_numpy(rng.integers(1, 4, m).astype(np.float32))
    layers = om.layers_from_temporal(ei, t, n, delta=delta, max_order=2, edge_weight=w)
    gen = torch.Generator().manual_seed(seed + 1)
    x, x_h = torch.randn(n, f, generator=gen), torch.randn(layers[2]["num_nodes"], f, generator=gen)
    y = torch.randint(0, 3, (n,), generator=gen)
    params = od.init_params(3, (f, f), hidden, seed=seed + 2)
    want = od.loss_and_grads(params, om.dbgnn_inputs(layers, 2, "last", x=x, x_h=x_h), y)
    return ei, t, w, x, x_h, y, params, want, layers


@pytest.mark.parametrize("dense_fo", [True, False])
def test_partition_path_world8_er_and_zipf_on_one_gpu(dense_fo, monkeypatch):
    """world size 8 with the REAL kernels — eight ranks as threads of this process sharing the one GPU
    (pathpyg_amd.distributed.ThreadWorld: device-to-device collectives; eight PROCESSES on one GPU spend minutes in context switches) —
    on an ER and a Zipf stream (weighted events) and a tiny one: the fully sharded build + the partitioned DBGNN step against the
    single-process oracle, features through row loaders.  The gloo transport itself is covered at world size 2 and 3 above."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    monkeypatch.setattr(pd, "FO_DENSE_HALO", dense_fo)          # first-order shard: every foreign node as halo (no discovery) / the discovered halo
    dev = torch.device("cuda:0")
    cases = [("er", _case(11, 20000, 300, 30, 6000, 64, [64, 64, 64], False), 300, 30, 64, [64, 64, 64]),
             ("zipf", _zipf_case(12, 20000, 300, 30, 6000, 64, [64, 64, 64]), 300, 30, 64, [64, 64, 64]),
             ("tiny", _case(13, 50, 20, 3, 60, 16, [16, 16, 16], False), 20, 3, 16, [16, 16, 16]),
             # ~12 events per node: the node-range partition on the node-by-node builder (no pair routing, no id exchange), plain and weighted
             ("er-sparse", _case(14, 7000, 600, 70, 7000, 64, [64, 64, 64], False), 600, 70, 64, [64, 64, 64]),
             ("er-sparse-weighted", _case(15, 5000, 450, 60, 6000, 32, [32, 32, 16], True), 450, 60, 32, [32, 32, 16])]
    for kind, (ei, t, w, x, x_h, y, params, want, layers), n, delta, f, hidden in cases:
        want_out, want_loss, want_grads = want
        attrs = {} if w is None else {"edge_weight": w.to(dev)}
        tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(dev), time=t.to(dev), num_nodes=n, **attrs))
        xd, xhd, yd = x.to(dev), x_h.to(dev), y.to(dev)

        def body(comm):
            shard = pd.build_dbgnn_shard(tg, delta, lambda rows: xd.index_select(0, rows), lambda rows: xhd.index_select(0, rows),
                                         lambda rows: yd.index_select(0, rows), comm)
            sz = pd.global_sizes(shard, comm)
            assert sz["U2"] == layers[2]["num_nodes"] and sz["A2"] == layers[2]["edge_index"].size(1), kind
            assert shard.ho.send_unique and shard.x_h.size(0) == shard.ho.n_src and shard.x.size(0) == shard.fo.n_src
            assert (shard.sizes.get("builder") == "fused") == (kind in ("tiny", "er-sparse", "er-sparse-weighted")), kind      # (hub nodes: generic kernels)
            net = pp.nn.DBGNN(num_classes=3, num_features=(f, f), hidden_dims=hidden).to(dev)
            net.load_state_dict(params)
            sharded = pd.ShardedDBGNN(net, comm)
            out = sharded(shard)
            assert_embeddings_close(out, want_out[shard.fo.lo: shard.fo.hi], what=kind)
            loss = sharded.loss(shard)
            loss.backward()
            pd.all_reduce_gradients(net, average=False, comm=comm)
            total = loss.detach().clone().reshape(1)
            comm.all_reduce_(total)
            torch.testing.assert_close(total.cpu()[0], want_loss, rtol=RTOL, atol=ATOL)
            for name, p in net.named_parameters():
                # (zipf: hub rows sum thousands of fp32 terms in another order than the oracle — entries that cancel to ~1e-3 of the
                #  typical magnitude carry that noise: 3e-5; every other stream: the north star's 1e-5)
                assert_gradients_close(p.grad, want_grads[name], f"{kind} {name}", rtol=3e-5 if kind == "zipf" else 1e-5)
            return "ok"

        assert pd.run_thread_world(8, body, dev) == ["ok"] * 8, kind


def _bench(extra, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    small = ["--events", "200000", "--nodes", "10000", "--span", "200000", "--delta", "20000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + extra, capture_output=True, text=True, timeout=timeout, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_partition_default_and_rccl_world1_and_gloo_world2(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    one = _bench(["--full"])
    assert one["n_gpus"] == 1 and one["scaling"] == "strong" and one["roofline"]["frac"] > 0 and one["lift_roofline"]["frac"] > 0
    assert one["aggregation_roofline"]["frac"] > 0 and one["config"]["E2"] > 0
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    small = ["--events", "200000", "--nodes", "10000", "--span", "200000", "--delta", "20000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    for nproc, extra in ((1, []), (2, ["--backend", "gloo", "--share-gpu", "--mode", "partition"])):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
                            "--master-port", str(port + nproc), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + small + extra,
                           capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert line["n_gpus"] == nproc and line["config"]["E2"] == one["config"]["E2"] and line["config"]["A2"] == one["config"]["A2"]
        assert abs(line["loss"] - one["loss"]) < 1e-3 * max(1.0, abs(one["loss"]))
        if nproc == 2:
            assert line["comm_bytes_per_step_rank0"]["exchange"] > 0 and line["comm_bytes_per_step_rank0"]["reduce_scatter"] > 0
    # the emulation (R ranks as threads on the one GPU) trains the same model on the same stream: same loss after the same steps
    emulated = _bench(["--emulate-ranks", "3"])
    assert emulated["emulated_ranks"] == 3 and emulated["E2"] == one["config"]["E2"]
    # the projection: per rank max(device, host) + blocking collectives + the replayed asynchronous ones; never below the slowest rank's compute
    assert emulated["clock"].startswith("events") and len(emulated["per_rank_device_ms"]) == 3 and min(emulated["per_rank_host_ms"]) > 0
    assert all(s_ >= 0 for s_ in emulated["per_rank_async_stall_ms"]) and emulated["async_timeline_rank1_last_step"]
    assert emulated["projected_ms_per_step"] >= emulated["max_rank_compute_ms"] > 0
    drained = _bench(["--emulate-ranks", "3", "--emulate-clock", "drain"])
    assert drained["clock"].startswith("drain") and abs(drained["loss"] - emulated["loss"]) < 1e-6 * max(1.0, abs(emulated["loss"]))
    assert abs(emulated["loss"] - one["loss"]) < 1e-3 * max(1.0, abs(one["loss"])), (emulated["loss"], one["loss"])
    # BASELINE configs[1] (2M events), forward pass at the initial weights: the 8-way sharded build + partitioned forward against the single-GPU path
    c1 = ["--warmup", "0", "--steps", "1", "--events", "2000000", "--nodes", "100000", "--span", "1000000", "--delta", "100000"]
    dump = tmp_path / "outputs"
    whole, split = _bench(c1 + ["--dump-outputs", str(dump)]), _bench(c1 + ["--emulate-ranks", "8"])
    assert split["E2"] == whole["config"]["E2"] and split["A2"] == whole["config"]["A2"] and split["U2"] == whole["config"]["U2"]
    assert abs(split["loss"] - whole["loss"]) < 1e-5 * abs(whole["loss"]), (split["loss"], whole["loss"])
    # a plain run: the headline line without what --full adds; --dump-outputs: the last timed step's loss, weights, gradients and plans
    assert whole["steps"] == 1 and whole["ms_per_step"] > 0 and whole["value"] > 0
    assert not {"lift_roofline", "aggregation_roofline", "api_path", "hub_streams", "multi_order", "cpu_baseline"} & set(whole)
    files = {f.name: np.load(f) for f in dump.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20
    assert abs(float(files["loss.npy"][0]) - whole["loss"]) < 1e-6 * abs(whole["loss"])
    assert any(k.startswith("param.") for k in files) and any(k.startswith("grad.") for k in files)
    fo_ptr = files["plan_fo.fwd_ptr.npy"]             # (10^5 + 1 entries: below the sampling threshold, written whole)
    assert fo_ptr.size == 100_001 and fo_ptr[0] == 0 and (np.diff(fo_ptr) >= 0).all() and {"plan_ho.fwd_idx.npy", "plan_ho.fwd_val.npy"} <= set(files)
    # the driver's command shape without a launcher: `python bench.py --gpus N` starts its own ranks
    self_launched = _bench(["--gpus", "2", "--backend", "gloo", "--share-gpu", "--mode", "partition"])
    assert self_launched["n_gpus"] == 2 and self_launched["config"]["E2"] == one["config"]["E2"] and self_launched["scaling"] == "strong"
    # default mode at 2 ranks: independent streams (the 2- / 4-rank split of ONE stream is link-bound on point-to-point xGMI), said so in the line
    auto = _bench(["--gpus", "2", "--backend", "gloo", "--share-gpu"])
    assert auto["n_gpus"] == 2 and auto["scaling"] == "weak" and "link-bound" in auto["mode_note"] and auto["value"] > 0


def _masked_reference(case, p, seed):
    """Single-process torch-CPU evaluation of the reference forward with the partition path's reproducible dropout masks."""
    import torch.nn.functional as F
    from oracle import dbgnn as od
    from oracle import model as om
    from pathpyg_amd.nn.sharded import dropout_mask
    ei, t, w, x, x_h, y, params, want, layers = _case(*case)
    data = om.dbgnn_inputs(layers, 2, "last", x=x, x_h=x_h)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    n, n_ho, n_gcn = data["num_nodes"], data["num_ho_nodes"], len(case[6]) - 1

    def run_stack(h, prefix, eidx, ew, tag):
        rows = torch.arange(h.size(0))
        for i in range(n_gcn):
            h = F.elu(od.gcn_conv(h * dropout_mask(rows, h.size(1), p, seed, tag + i), eidx, ew, leaves[f"{prefix}.{i}.lin.weight"], leaves[f"{prefix}.{i}.bias"]))
        return h
    hx = run_stack(x, "first_order_layers", data["edge_index"], data["edge_weights"], 0) * 1.0
    hh = run_stack(x_h, "higher_order_layers", data["edge_index_higher_order"], data["edge_weights_higher_order"], 64)
    hx = hx * dropout_mask(torch.arange(n), hx.size(1), p, seed, 32)
    hh = hh * dropout_mask(torch.arange(n_ho), hh.size(1), p, seed, 96)
    z = F.elu(od.bipartite_op(hh, hx, data["bipartite_edge_index"], n, leaves["bipartite_layer.lin1.weight"], leaves["bipartite_layer.lin1.bias"],
                              leaves["bipartite_layer.lin2.weight"], leaves["bipartite_layer.lin2.bias"]))
    out = (z * dropout_mask(torch.arange(n), z.size(1), p, seed, 128)) @ leaves["lin.weight"].t() + leaves["lin.bias"]
    loss = F.cross_entropy(out, y)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2]], ids=["F16", "F64", "F128"])
def test_partition_path_dropout_matches_masked_reference(case):
    """Training-mode dropout on the partitioned path with the HIP kernels (world size 1): loss and every gradient against the reference forward
    evaluated on the CPU with the same (seed, tag, global row, column) masks."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    dev, p = torch.device("cuda:0"), 0.4
    ei, t, w, x, x_h, y, params, want, layers = _case(*case)
    attrs = {} if w is None else {"edge_weight": w.to(dev)}
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(dev), time=t.to(dev), num_nodes=case[2], **attrs))
    comm = pd.Comm()
    shard = pd.build_dbgnn_shard(tg, case[3], x.to(dev), x_h.to(dev), y.to(dev), comm)
    net = pp.nn.DBGNN(num_classes=3, num_features=(case[5], case[5]), hidden_dims=case[6], p_dropout=p).to(dev)
    net.load_state_dict(params)
    net.train()
    torch.manual_seed(5)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64).item())
    torch.manual_seed(5)
    loss = pd.ShardedDBGNN(net, comm).loss(shard)
    loss.backward()
    want_loss, want_grads = _masked_reference(case, p, seed)
    torch.testing.assert_close(loss.detach().cpu(), want_loss, rtol=RTOL, atol=ATOL)
    for name, prm in net.named_parameters():
        assert_gradients_close(prm.grad, want_grads[name], name)


@pytest.mark.parametrize("world", [3, 8])
def test_partition_path_dropout_on_ranks_sharing_one_gpu(world):
    """Training-mode dropout across 3 and 8 ranks (HIP kernels; the ranks are threads of this process, ThreadWorld): the owner's layer kernel drops
    its rows in the epilogue with the GLOBAL row id (drop_row0 = the shard's first row) before they are exchanged; loss and gradients equal
    the single-process evaluation with the same masks."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    dev, p = torch.device("cuda:0"), 0.4
    torch.manual_seed(5)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,), dtype=torch.int64).item())
    for case in (CASES[0], CASES[1], CASES[2], CASES[6]):          # (the last one: node-range partition on the node-by-node builder; its halo ids are fetched lazily for the masks)
        ei, t, w, x, x_h, y, params, want, layers = _case(*case)
        want_loss, want_grads = _masked_reference(case, p, seed)
        attrs = {} if w is None else {"edge_weight": w.to(dev)}
        tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(dev), time=t.to(dev), num_nodes=case[2], **attrs))

        def body(comm):
            shard = pd.build_dbgnn_shard(tg, case[3], x.to(dev), x_h.to(dev), y.to(dev), comm)
            net = pp.nn.DBGNN(num_classes=3, num_features=(case[5], case[5]), hidden_dims=case[6], p_dropout=p).to(dev)
            net.load_state_dict(params)
            net.train()
            torch.manual_seed(5)                       # every rank draws the same seed (the model agrees on the maximum)
            loss = pd.ShardedDBGNN(net, comm).loss(shard)
            loss.backward()
            pd.all_reduce_gradients(net, average=False, comm=comm)
            total = loss.detach().clone().reshape(1)
            comm.all_reduce_(total)
            torch.testing.assert_close(total.cpu()[0], want_loss, rtol=RTOL, atol=ATOL)
            for name, prm in net.named_parameters():
                assert_gradients_close(prm.grad, want_grads[name], f"{case[5]} {name}")
            return "ok"

        assert pd.run_thread_world(world, body, dev) == ["ok"] * world
