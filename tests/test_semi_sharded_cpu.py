"""The semi-supervised loop on a PARTITIONED DBGNN without a GPU: node splits on shards, the masked / class-weighted loss and the scores
across ranks (one small all-reduce each), implicit one-hot features on shards.  The collectives run for real — gloo processes at world 2 and
3, an 8-thread ``ThreadWorld`` — and the device operations are the torch-CPU stand-ins of tests/cpu_ops.py + tests/cpu_ops_semi.py.

Reference: the oracle's forward (oracle/dbgnn.py) in FLOAT64 on explicit features — ``torch.eye`` for the implicit default — with
``F.cross_entropy(out[mask], y[mask], weight=, ignore_index=, reduction=)`` written here, and numpy's confusion matrix on its logits.
Bars: tests/tolerance.py (1e-5 element-wise for logits and gradients) and RTOL, ATOL = 1e-5, 2e-6 for losses."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests.tolerance import assert_embeddings_close, assert_gradients_close

RTOL, ATOL = 1e-5, 2e-6
CLASSES, HIDDEN, FEAT = 3, [12, 10, 6], 8
WEIGHT = torch.tensor([0.5, 2.0, 1.25])
IGNORE = -1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _problem(kind):
    """A small event stream, its layers (oracle), labels with a few ignored nodes, a train / test split, explicit features."""
    from oracle import model as om
    m, n, delta, span = {"edge": (4000, 80, 12, 1500), "node": (2000, 80, 30, 2400), "tiny": (40, 5, 4, 60)}[kind]
    rng = np.random.default_rng({"edge": 61, "node": 67, "tiny": 71}[kind])
    ei = torch.from_numpy(rng.integers(0, n, (2, m)))
    t = torch.from_numpy(np.sort(rng.integers(0, span, m)))
    w = torch.from_numpy((rng.random(m) + 0.5).astype(np.float32)) if kind == "edge" else None
    layers = om.layers_from_temporal(ei, t, n, delta=delta, max_order=2, edge_weight=w)
    n_ho = layers[2]["num_nodes"]
    gen = torch.Generator().manual_seed(9)
    y = torch.randint(0, CLASSES, (n,), generator=gen)
    y[torch.randperm(n, generator=gen)[: max(n // 10, 1)]] = IGNORE
    where = torch.randint(0, 3, (n,), generator=gen)
    masks = {"train": where == 0, "test": where == 1, "low": torch.arange(n) < min(3, n), "none": torch.zeros(n, dtype=torch.bool)}
    return {"ei": ei, "t": t, "w": w, "n": n, "n_ho": n_ho, "delta": delta, "layers": layers, "y": y, "masks": masks,
            "x": torch.randn(n, FEAT, generator=gen), "x_h": torch.randn(n_ho, FEAT, generator=gen)}


def _reference(params, inputs, y, mask, reduction):
    """(logits, loss, gradients) in float64: the oracle's forward + torch's masked, weighted cross-entropy."""
    from oracle import dbgnn as od
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    data = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in inputs.items()}
    out = od.forward(leaves, data)
    loss = F.cross_entropy(out[mask], y[mask], weight=WEIGHT.double(), ignore_index=IGNORE, reduction=reduction)
    loss.backward()
    return out.detach(), loss.detach(), {k: v.grad for k, v in leaves.items()}


def _numpy_scores(logits, y, mask):
    z, t = logits.numpy(), y.numpy()
    keep = mask.numpy() & (t != IGNORE)
    conf = np.zeros((CLASSES, CLASSES), dtype=np.int64)
    np.add.at(conf, (t[keep], z[keep].argmax(1)), 1)
    return conf, float(np.trace(conf) / max(conf.sum(), 1))


def _shard(pp, pd, prob, comm, ops, builder, implicit, y=None):
    y = prob["y"] if y is None else y
    x, x_h = (None, None) if implicit else (prob["x"], prob["x_h"])
    if builder == "bundle":
        from oracle import model as om
        from pathpyg_amd.data import Identity
        bundle = om.dbgnn_inputs(prob["layers"], 2, "last", x=prob["x"], x_h=prob["x_h"])
        if implicit:
            bundle.update(x=Identity(prob["n"]), x_h=Identity(prob["n_ho"]))
        data = pp.Data(**bundle, y=y, train_mask=prob["masks"]["train"], test_mask=prob["masks"]["test"])
        n = prob["n"]
        cuts = None if comm.world < 3 else [0] + [(n * r) // (comm.world - 1) for r in range(comm.world - 1)] + [n]      # rank 0 owns NO node
        shard = pd.shard_dbgnn_bundle(data, comm, ops, fo_cuts=cuts)
        assert set(shard.masks) == {"train_mask", "test_mask"} and (comm.world < 3 or comm.rank or shard.fo.n_own == 0)
        if implicit:
            assert data.is_identity("x") and isinstance(data.peek("x"), Identity) and data.peek("x").value is None      # nothing was resolved
        lo, hi = shard.fo.lo, shard.fo.hi
        shard.masks.update({k: v[lo:hi] for k, v in prob["masks"].items()})
        return shard
    tg = type("G", (), {})()
    tg.data = pp.Data(edge_index=prob["ei"], time=prob["t"], num_nodes=prob["n"], **({} if prob["w"] is None else {"edge_weight": prob["w"]}))
    loaders = {k: (v if k == "train" else (lambda rows, v=v: v.index_select(0, rows))) for k, v in prob["masks"].items()}
    return pd.build_dbgnn_shard(tg, prob["delta"], x, x_h, lambda rows: y.index_select(0, rows), comm, ops, masks=loaders)


def _scenario(comm, kind, builder, node_ops):
    """Everything the issue lists, with collectives through ``comm``; every assertion runs on every rank."""
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    from oracle import dbgnn as od
    from oracle import model as om
    from tests.cpu_ops_semi import CpuOpsNodeSemi, CpuOpsSemi
    ops = CpuOpsNodeSemi() if node_ops else CpuOpsSemi()
    prob = _problem(kind)
    n, n_ho, y, masks = prob["n"], prob["n_ho"], prob["y"], prob["masks"]
    train = "train_mask" if builder == "bundle" else "train"
    test = "test_mask" if builder == "bundle" else "test"
    owned = []
    for implicit in (False, True):
        feats = (n, n_ho) if implicit else (FEAT, FEAT)
        params = od.init_params(CLASSES, feats, HIDDEN, seed=5)
        inputs = om.dbgnn_inputs(prob["layers"], 2, "last", x=None if implicit else prob["x"], x_h=None if implicit else prob["x_h"])
        net = pp.nn.DBGNN(num_classes=CLASSES, num_features=feats, hidden_dims=HIDDEN)
        net.load_state_dict(params)
        sharded = pd.ShardedDBGNN(net, comm, ops=ops)
        shard = _shard(pp, pd, prob, comm, ops, builder, implicit)
        if node_ops:
            assert shard.sizes.get("builder") == "fused"
        lo, hi = shard.fo.lo, shard.fo.hi
        owned.append(hi - lo)
        assert (shard.x is None and shard.x_h is None) == implicit
        assert builder == "bundle" or pd.global_sizes(shard, comm)["U2"] == n_ho              # (reads the shard's device: x may be None)
        if implicit:
            assert torch.equal(shard.fo.rows[: hi - lo], torch.arange(lo, hi)) and shard.fo.rows.numel() == shard.fo.n_src
            assert shard.ho.rows.numel() == shard.ho.n_src and int(shard.ho.rows.unique().numel()) == shard.ho.n_src
        assert all(v.dtype == torch.bool and v.shape == (hi - lo,) for v in shard.masks.values())
        assert torch.equal(shard.masks[train], masks["train"][lo:hi]) and torch.equal(shard.y, y[lo:hi])
        for reduction in ("mean", "sum"):
            want_out, want_loss, want_grads = _reference(params, inputs, y, masks["train"], reduction)
            net.zero_grad()
            share = sharded.loss(shard, mask=train, weight=WEIGHT, ignore_index=IGNORE, reduction=reduction)
            share.backward()
            pd.all_reduce_gradients(net, average=False, comm=comm)
            total = comm.all_reduce_(share.detach().double().reshape(1).clone())[0]
            torch.testing.assert_close(total, want_loss, rtol=RTOL, atol=ATOL)
            for name, prm in net.named_parameters():
                assert_gradients_close(prm.grad, want_grads[name], f"{builder}/{kind} implicit={implicit} {reduction} {name}")
        # a bool tensor instead of a key; a split in which only the lowest ids are selected (most ranks own no selected node)
        want_out, want_loss, want_grads = _reference(params, inputs, y, masks["low"], "mean")
        net.zero_grad()
        share = sharded.loss(shard, mask=masks["low"][lo:hi], weight=WEIGHT, ignore_index=IGNORE)
        share.backward()
        local_selected = int((masks["low"][lo:hi] & (y[lo:hi] != IGNORE)).sum())
        if local_selected == 0:          # (its weight gradients need not vanish: the peers' rows reach its layers through the halo exchange)
            assert float(share.detach()) == 0.0
        pd.all_reduce_gradients(net, average=False, comm=comm)
        torch.testing.assert_close(comm.all_reduce_(share.detach().double().reshape(1).clone())[0], want_loss, rtol=RTOL, atol=ATOL)
        for name, prm in net.named_parameters():
            assert_gradients_close(prm.grad, want_grads[name], f"{builder}/{kind} implicit={implicit} low {name}")
        # logits and scores
        net.zero_grad()
        assert_embeddings_close(sharded(shard), want_out[lo:hi], what=f"{builder}/{kind} implicit={implicit} logits")
        scores = sharded.evaluate(shard, mask=test, ignore_index=IGNORE)
        # (the reference logits decide the argmax: the test split has no near-tie at these sizes — checked by the margin below)
        conf, acc = _numpy_scores(want_out, y, masks["test"])
        top2 = want_out[masks["test"]].topk(2, dim=1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-4
        assert np.array_equal(scores["confusion"].numpy(), conf) and scores["accuracy"] == pytest.approx(acc, abs=1e-12)
        assert torch.equal(scores["support"], torch.from_numpy(conf.sum(1)))
        # an empty global selection: NaN mean, all-zero gradients
        net.zero_grad()
        empty = sharded.loss(shard, mask="none" if builder != "bundle" else masks["none"][lo:hi], weight=WEIGHT, ignore_index=IGNORE)
        empty.backward()
        assert bool(torch.isnan(empty))
        assert all(prm.grad is not None and not bool(prm.grad.any()) and bool(torch.isfinite(prm.grad).all()) for prm in net.parameters())
        # a selected target outside [0, C) on ONE rank: every rank raises, and the next collective still completes
        bad_y = y.clone()
        bad_node = int(torch.nonzero(masks["train"]).flatten()[-1])
        bad_y[bad_node] = CLASSES + 4
        bad_shard = _shard(pp, pd, prob, comm, ops, builder, implicit, y=bad_y)
        with pytest.raises(IndexError):
            sharded.loss(bad_shard, mask=train, ignore_index=IGNORE)
        with pytest.raises(IndexError):
            sharded.evaluate(bad_shard, mask=train, ignore_index=IGNORE)
        assert int(comm.all_reduce_(torch.ones(1, dtype=torch.int64))[0]) == comm.world
    return owned


def _gloo_worker(rank, world, port, results, kind, builder, node_ops):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        from pathpyg_amd import distributed as pd
        _scenario(pd.Comm(), kind, builder, node_ops)
        results[rank] = "ok"
    finally:
        dist.destroy_process_group()


def _spawn(world, *args, timeout=300):
    ctx = mp.get_context("spawn")
    results = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, results) + args) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
        assert p.exitcode == 0
    assert dict(results) == {r: "ok" for r in range(world)}


CASES = [("edge", "bundle", False), ("edge", "stream", False), ("node", "stream", True)]


@pytest.mark.parametrize("kind,builder,node_ops", CASES)
@pytest.mark.parametrize("world", [2, 3])
def test_masked_loss_scores_and_implicit_features_on_gloo_ranks(world, kind, builder, node_ops):
    _spawn(world, kind, builder, node_ops)


@pytest.mark.parametrize("kind,builder,node_ops", CASES + [("tiny", "stream", False), ("tiny", "stream", True)])
def test_masked_loss_scores_and_implicit_features_on_eight_thread_ranks(kind, builder, node_ops):
    """8 ranks as threads.  The bundle case cuts rank 0 out of the first-order nodes; the 5-node stream leaves at least three ranks without one."""
    from pathpyg_amd import distributed as pd
    owned = pd.run_thread_world(8, lambda comm: _scenario(comm, kind, builder, node_ops))
    if builder == "bundle" or kind == "tiny":
        assert any(o == [0, 0] for o in owned)
    assert sum(o[0] for o in owned) == _problem(kind)["n"]


def test_shards_refuse_what_they_cannot_serve():
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    from oracle import dbgnn as od
    from tests.cpu_ops_semi import CpuOpsSemi
    prob = _problem("tiny")
    comm = pd.Comm()
    shard = _shard(pp, pd, prob, comm, CpuOpsSemi(), "stream", True)
    net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(FEAT, FEAT), hidden_dims=HIDDEN)      # first layers that do not fit an identity
    sharded = pd.ShardedDBGNN(net, comm, ops=CpuOpsSemi())
    with pytest.raises(ValueError, match="one-hot"):
        sharded(shard)
    fit = pp.nn.DBGNN(num_classes=CLASSES, num_features=(prob["n"], prob["n_ho"]), hidden_dims=HIDDEN)
    fit.load_state_dict(od.init_params(CLASSES, (prob["n"], prob["n_ho"]), HIDDEN, seed=1))
    sharded = pd.ShardedDBGNN(fit, comm, ops=CpuOpsSemi())
    with pytest.raises(KeyError, match="validation"):
        sharded.loss(shard, mask="validation")
    with pytest.raises(ValueError, match="bool"):
        sharded.loss(shard, mask=torch.ones(prob["n"] + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="reduction"):
        sharded.loss(shard, mask="train", reduction="none")
    clean = _shard(pp, pd, prob, comm, CpuOpsSemi(), "stream", True, y=prob["y"].clamp(min=0))
    assert bool(torch.isfinite(sharded.loss(clean)))                                      # the keyword-free loss runs on implicit shards too
