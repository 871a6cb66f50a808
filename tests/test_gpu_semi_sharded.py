"""The semi-supervised loop on a PARTITIONED DBGNN with the real HIP kernels: the row-mapped one-hot first layer
(pp_spmm_diag_drop_map_f32), the masked / class-weighted loss and the scores across ranks (pp_cross_entropy_masked_sums_f32 +
pp_masked_finish_f32, pp_confusion_f32), implicit one-hot features on shards, and the whole training loop on 3 ranks.  Ranks > 1 are threads
of this process on the one GPU (``run_thread_world``).

References (never the code under test): the pre-existing kernels for the bit-equality checks of the new one; the oracle's forward
(oracle/dbgnn.py) in float64 on an explicit ``torch.eye`` with torch's ``F.cross_entropy(..., weight=, ignore_index=, reduction=)``; for
dropout the masked reference of tests/test_gpu_one_hot.py restated below; numpy for the confusion matrix.
Bars: tests/tolerance.py at 1e-5 for logits and gradients, RTOL, ATOL = 1e-5, 2e-6 for losses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.tolerance import assert_embeddings_close, assert_gradients_close, gradient_rtol_needed

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 2e-6
DEV = torch.device("cuda:0")
CLASSES, IGNORE = 3, -1
WEIGHT = torch.tensor([0.5, 2.0, 1.25])


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
def _csr(gen, n_rows, entries, n_cols, long_row=None):
    """Random CSR (ptr int32 [n_rows + 1], idx int32 into [0, n_cols), val fp32); ``long_row``: that row alone gets 200 entries more."""
    rows = torch.randint(0, n_rows, (entries,), generator=gen)
    if long_row is not None:
        rows = torch.cat((rows, torch.full((200,), long_row, dtype=torch.int64)))
    rows = rows.sort().values
    ptr = torch.zeros(n_rows + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    idx = torch.randint(0, n_cols, (rows.numel(),), generator=gen).int()
    val = torch.rand(rows.numel(), generator=gen) + 0.25
    return ptr.to(DEV), idx.to(DEV), val.to(DEV)


KERNEL_CASES = [(1, 1, 4, None, None), (65, 300, 16, None, None), (4097, 30_000, 64, 70_001, None), (300, 9000, 100, None, 7),
                (1000, 5000, 256, None, None)]


@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("n_rows,entries,f,n_big,long_row", KERNEL_CASES, ids=[f"r{c[0]}_F{c[2]}" for c in KERNEL_CASES])
def test_row_mapped_kernel_equals_the_unmapped_kernel_bit_for_bit(n_rows, entries, f, n_big, long_row, p):
    """where 1 and 2.  Identity map: the bits of pp_spmm_diag_drop_f32.  A random injective, non-monotone map into a larger id space (70 001
    ids in one case: the hash index g * n + g passes 2^32): the bits of the existing kernel on the gathered copy, with the factors of the GLOBAL
    ids (``dropout_mask_diagonal``, the torch statement of the hash) multiplied into its coefficients beforehand — the one fp32 product the
    kernel makes; where 2: its output times the factor, scattered by the map, every other row of Y exactly zero."""
    _need_gpu()
    from pathpyg_amd import _hip
    from pathpyg_amd.nn.sharded import dropout_mask_diagonal
    gen = torch.Generator().manual_seed(n_rows + f)
    seed, tag = 1234567, 64
    ptr, idx, val = _csr(gen, n_rows, entries, n_rows, long_row)
    if long_row is not None:
        assert int((ptr[1:] - ptr[:-1]).max()) > 64                                  # more entries than the widest lane group
    self_coef = (torch.rand(n_rows, generator=gen) + 0.1).to(DEV)
    bias = torch.randn(f, generator=gen).to(DEV)
    x = torch.randn(n_rows, f, generator=gen).to(DEV)
    # ---- identity map
    ident = torch.arange(n_rows, device=DEV)
    for where, b, act in ((1, bias, True), (2, None, False)):
        want = _hip.spmm_diag_drop(ptr, idx, val, n_rows, x, self_coef, b, act, where, n_rows, p, seed, tag)
        got = _hip.spmm_diag_drop_map(ptr, idx, val, n_rows, x, self_coef, b, act, where, ident, n_rows, p, seed, tag)
        assert torch.equal(got, want), f"identity map, where {where}"
    # ---- an injective map into a larger id space
    n = n_big if n_big is not None else 2 * n_rows + 7
    row_map = torch.randperm(n, generator=gen)[:n_rows].to(DEV)
    assert n_rows < 3 or not bool((row_map[1:] > row_map[:-1]).all())                   # non-monotone, as the send-order shards are
    d = dropout_mask_diagonal(row_map, n, p, seed, tag) if p > 0 else torch.ones(n_rows, device=DEV)
    x_big = torch.randn(n, f, generator=gen).to(DEV)
    gathered = x_big.index_select(0, row_map)
    want = _hip.spmm_diag_drop(ptr, idx, val * d[idx.long()], n_rows, gathered, self_coef * d, bias, True, 1, n_rows, 0.0, seed, tag)
    out = torch.full((n_rows, f), float("nan"), device=DEV)
    got = _hip.spmm_diag_drop_map(ptr, idx, val, n_rows, x_big, self_coef, bias, True, 1, row_map, n, p, seed, tag, out=out)
    assert got is out and torch.equal(got, want), "mapped, where 1"
    plain = _hip.spmm_diag_drop(ptr, idx, val, n_rows, x, self_coef, None, False, 2, n_rows, 0.0, seed, tag)
    want = torch.zeros(n, f, device=DEV)
    want[row_map] = plain * d.unsqueeze(1)
    got = _hip.spmm_diag_drop_map(ptr, idx, val, n_rows, x, self_coef, None, False, 2, row_map, n, p, seed, tag)
    assert torch.equal(got, want), "mapped, where 2"
    untouched = torch.ones(n, dtype=torch.bool, device=DEV)
    untouched[row_map] = False
    assert not bool(got[untouched].any())


def test_row_mapped_backward_on_a_rectangular_share():
    """where 2 with more source slots than owned rows (a rank's [owned | halo] space): the halo slots get no self term — their rows are the
    bits of the plain CSR kernel — and the owned slots are the bits of the square kernel on the first rows of the same CSR."""
    _need_gpu()
    from pathpyg_amd import _hip
    gen = torch.Generator().manual_seed(11)
    n_own, n_src, f, n = 130, 333, 32, 1000
    ptr, idx, val = _csr(gen, n_src, 4000, n_own)
    self_coef = (torch.rand(n_own, generator=gen) + 0.1).to(DEV)
    dpre = torch.randn(n_own, f, generator=gen).to(DEV)
    row_map = torch.randperm(n, generator=gen)[:n_src].to(DEV)
    got = _hip.spmm_diag_drop_map(ptr, idx, val, n_src, dpre, self_coef, None, False, 2, row_map, n, 0.0, 1, 0, n_self=n_own)
    halo = _hip.spmm(ptr, idx, val, n_src, dpre)[n_own:]
    own = _hip.spmm_diag_drop(ptr[: n_own + 1].contiguous(), idx, val, n_own, dpre, self_coef, None, False, 2, n_own, 0.0, 1, 0)
    assert torch.equal(got[row_map[n_own:]], halo) and torch.equal(got[row_map[:n_own]], own)
    with pytest.raises(IndexError):                                                      # ids outside [0, n) are refused before any launch
        _hip.spmm_diag_drop_map(ptr, idx, val, n_src, dpre, self_coef, None, False, 2, row_map + n, n, 0.0, 1, 0, n_self=n_own)


# ------------------------------------------------------------------------------------------------------------------ shared problems
def _stream(seed, m, n, delta, span, weighted):
    from oracle import model as om
    rng = np.random.default_rng(seed)
    ei = torch.from_numpy(rng.integers(0, n, (2, m)))
    t = torch.from_numpy(np.sort(rng.integers(0, span, m)))
    w = torch.from_numpy(rng.integers(1, 4, m).astype(np.float32)) if weighted else None
    layers = om.layers_from_temporal(ei, t, n, delta=delta, max_order=2, edge_weight=w)
    gen = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, CLASSES, (n,), generator=gen)
    y[torch.randperm(n, generator=gen)[: n // 10]] = IGNORE
    where = torch.randint(0, 3, (n,), generator=gen)
    return {"ei": ei, "t": t, "w": w, "n": n, "n_ho": layers[2]["num_nodes"], "delta": delta, "layers": layers, "y": y,
            "masks": {"train": where == 0, "test": where == 1, "none": torch.zeros(n, dtype=torch.bool)}}


def _graph(pp, prob):
    attrs = {} if prob["w"] is None else {"edge_weight": prob["w"].to(DEV)}
    return pp.TemporalGraph(pp.Data(edge_index=prob["ei"].to(DEV), time=prob["t"].to(DEV), num_nodes=prob["n"], **attrs))


def _reference(params, inputs, y, mask, reduction="mean", weight=WEIGHT, ignore_index=IGNORE, p=0.0, seed=0):
    """(logits, loss, gradients) in float64 on the CPU: the reference forward (dbgnn.py:131-150) — with the masks of ``dropout_mask`` at every
    site when ``p`` > 0, as tests/test_gpu_one_hot.py::_masked_reference — and torch's masked, weighted cross-entropy."""
    from oracle import dbgnn as od
    import pathpyg_amd.nn.dbgnn as mod
    from pathpyg_amd.nn.sharded import dropout_mask
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    cpu = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in inputs.items()}
    drop = (lambda t, tag: t * dropout_mask(torch.arange(t.size(0)), t.size(1), p, seed, tag).double()) if p > 0 else (lambda t, tag: t)
    n_gcn = sum(1 for k in params if k.startswith("first_order_layers.") and k.endswith(".bias"))
    x, x_h = cpu["x"], cpu["x_h"]
    for i in range(n_gcn):
        x = F.elu(od.gcn_conv(drop(x, mod.TAG_FO + i), cpu["edge_index"], cpu["edge_weights"], leaves[f"first_order_layers.{i}.lin.weight"],
                              leaves[f"first_order_layers.{i}.bias"]))
    x = drop(x, mod.TAG_FO_OUT)
    for i in range(n_gcn):
        x_h = F.elu(od.gcn_conv(drop(x_h, mod.TAG_HO + i), cpu["edge_index_higher_order"], cpu["edge_weights_higher_order"],
                                leaves[f"higher_order_layers.{i}.lin.weight"], leaves[f"higher_order_layers.{i}.bias"]))
    x_h = drop(x_h, mod.TAG_HO_OUT)
    x = F.elu(od.bipartite_op(x_h, x, cpu["bipartite_edge_index"], cpu["num_nodes"], leaves["bipartite_layer.lin1.weight"],
                              leaves["bipartite_layer.lin1.bias"], leaves["bipartite_layer.lin2.weight"], leaves["bipartite_layer.lin2.bias"]))
    out = drop(x, mod.TAG_HEAD) @ leaves["lin.weight"].t() + leaves["lin.bias"]
    loss = F.cross_entropy(out[mask], y[mask], weight=None if weight is None else weight.double(),
                           ignore_index=-100 if ignore_index is None else ignore_index, reduction=reduction)
    loss.backward()
    return out.detach(), loss.detach(), {k: v.grad for k, v in leaves.items()}


def _numpy_confusion(logits, y, mask):
    z, t = logits.numpy(), y.numpy()
    keep = mask.numpy() & (t != IGNORE)
    conf = np.zeros((CLASSES, CLASSES), dtype=np.int64)
    np.add.at(conf, (t[keep], z[keep].argmax(1)), 1)
    return conf


def _gradients_close(grads, want_grads, what):
    """``assert_gradients_close`` (1e-5) for every parameter, the needed rtol of each printed first (``pytest -s``) and ALL misses reported."""
    misses = []
    for name, g in grads.items():
        needed = gradient_rtol_needed(g, want_grads[name])
        print(f"[gradient] {what} {name}: needs rtol {needed:.2e}")
        try:
            assert_gradients_close(g, want_grads[name], f"{what} {name}")
        except AssertionError as exc:
            misses.append(str(exc))
    assert not misses, "\n".join(misses)


def _assert_against(results, want_out, want_loss, want_grads, what):
    """``results``: per rank ``{"out", "lo", "hi", "share", "grads"}`` (gradients already all-reduced)."""
    assert sum(r["hi"] - r["lo"] for r in results) == want_out.size(0)
    got = torch.cat([r["out"].cpu() for r in sorted(results, key=lambda r: r["lo"])])
    assert_embeddings_close(got, want_out, what=f"{what} logits")
    total = sum(float(r["share"]) for r in results)
    torch.testing.assert_close(torch.tensor(total, dtype=torch.float64), want_loss, rtol=RTOL, atol=ATOL)
    for r in results[:1]:                    # (all-reduced: every rank holds the same gradients — checked below)
        _gradients_close(r["grads"], want_grads, what)
    for r in results[1:]:
        assert all(torch.equal(g, results[0]["grads"][name]) for name, g in r["grads"].items())


def _step(pd, sharded, shard, net, comm, **loss_kw):
    net.zero_grad()
    out = sharded(shard).detach()
    share = sharded.loss(shard, **loss_kw)
    share.backward()
    pd.all_reduce_gradients(net, average=False, comm=comm)
    return {"out": out, "lo": shard.fo.lo, "hi": shard.fo.hi, "share": share.detach().double().cpu(),
            "grads": {k: v.grad.detach().clone() for k, v in net.named_parameters()}}


# ------------------------------------------------------------------------------------------------------------------ 2. the loss
def test_world1_masked_loss_is_the_single_gpu_loss_bit_for_bit():
    _need_gpu()
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    from pathpyg_amd.nn.sharded import HipOps, _ShardedMaskedLoss
    from oracle import dbgnn as od
    prob = _stream(3, 6000, 60, 12, 900, True)
    f, hidden = 16, [32, 32, 16]
    gen = torch.Generator().manual_seed(2)
    x, x_h = torch.randn(prob["n"], f, generator=gen), torch.randn(prob["n_ho"], f, generator=gen)
    comm = pd.Comm()
    masks = {k: v.to(DEV) for k, v in prob["masks"].items()}
    shard = pd.build_dbgnn_shard(_graph(pp, prob), prob["delta"], x.to(DEV), x_h.to(DEV), prob["y"].to(DEV), comm, masks=masks)
    assert set(shard.masks) == set(masks) and all(torch.equal(shard.masks[k], masks[k]) for k in masks)
    net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(f, f), hidden_dims=hidden).to(DEV)
    net.load_state_dict(od.init_params(CLASSES, (f, f), hidden, seed=5))
    sharded = pd.ShardedDBGNN(net, comm)
    weight = WEIGHT.to(DEV)
    logits = sharded(shard).detach()
    for kw in ({"mask": "train", "ignore_index": IGNORE}, {"mask": "train", "weight": weight, "ignore_index": IGNORE}, {"mask": masks["test"], "ignore_index": IGNORE, "reduction": "sum"},
               {"weight": weight, "ignore_index": IGNORE}, {"mask": "none"}):
        plain = dict(kw, mask=masks[kw["mask"]] if isinstance(kw.get("mask"), str) else kw.get("mask"))
        got = sharded.loss(shard, **kw)
        want = pp.nn.cross_entropy(logits, shard.y, **plain)
        assert torch.equal(got.detach(), want) or (bool(torch.isnan(got)) and bool(torch.isnan(want))), kw
        a, b = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
        share, counts = _ShardedMaskedLoss.apply(a, shard.y, plain.get("mask"), kw.get("weight"), kw.get("ignore_index"), kw.get("reduction", "mean") == "mean",
                                                 comm, HipOps())
        (share * 3.0).backward()
        (pp.nn.cross_entropy(b, shard.y, **plain) * 3.0).backward()
        assert torch.equal(a.grad, b.grad) and int(counts[1]) == 0, kw
    scores, want = sharded.evaluate(shard, mask="test", ignore_index=IGNORE), pp.nn.evaluate(logits, shard.y, mask=masks["test"], ignore_index=IGNORE)
    assert torch.equal(scores["confusion"], want["confusion"]) and {k: v for k, v in scores.items() if isinstance(v, float)} == \
        {k: v for k, v in want.items() if isinstance(v, float)}
    bad = shard.y.clone()
    bad[int(torch.nonzero(masks["train"]).flatten()[0])] = CLASSES
    shard.y = bad
    with pytest.raises(IndexError):
        sharded.loss(shard, mask="train")
    with pytest.raises(IndexError):
        sharded.evaluate(shard, mask="train")


LOSS_CASES = {"F16-weighted-events": ((3, 6000, 60, 12, 900, True), 16, [32, 32, 16], None),
              "node-range-fused-builder": ((9, 4000, 400, 60, 6000, False), 64, [64, 64, 64], "fused")}
_LOSS_REFERENCE = {}


def _loss_problem(name):
    """Problem + float64 references, computed once and shared by the world sizes."""
    if name not in _LOSS_REFERENCE:
        from oracle import dbgnn as od
        from oracle import model as om
        stream, f, hidden, builder = LOSS_CASES[name]
        prob = _stream(*stream)
        gen = torch.Generator().manual_seed(2)
        x, x_h = torch.randn(prob["n"], f, generator=gen), torch.randn(prob["n_ho"], f, generator=gen)
        params = od.init_params(CLASSES, (f, f), hidden, seed=5)
        inputs = om.dbgnn_inputs(prob["layers"], 2, "last", x=x, x_h=x_h)
        want = {r: _reference(params, inputs, prob["y"], prob["masks"]["train"], r) for r in ("mean", "sum")}
        # the scores are compared through the reference's argmax: rows whose two largest reference logits nearly tie leave the test split
        top2 = want["mean"][0].topk(2, dim=1).values
        prob["masks"]["test"] = prob["masks"]["test"] & ((top2[:, 0] - top2[:, 1]) > 1e-4)
        _LOSS_REFERENCE[name] = (prob, f, hidden, builder, x, x_h, params, want)
    return _LOSS_REFERENCE[name]


@pytest.mark.parametrize("name", list(LOSS_CASES))
@pytest.mark.parametrize("world", [3, 8])
def test_masked_weighted_loss_and_scores_across_ranks(world, name):
    _need_gpu()
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    prob, f, hidden, builder, x, x_h, params, want = _loss_problem(name)
    tg, weight = _graph(pp, prob), WEIGHT.to(DEV)
    masks = {k: v.to(DEV) for k, v in prob["masks"].items()}

    def body(comm):
        shard = pd.build_dbgnn_shard(tg, prob["delta"], x.to(DEV), x_h.to(DEV), prob["y"].to(DEV), comm, masks=masks)
        assert builder is None or shard.sizes.get("builder") == builder
        net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(f, f), hidden_dims=hidden).to(DEV)
        net.load_state_dict(params)
        sharded = pd.ShardedDBGNN(net, comm)
        res = {r: _step(pd, sharded, shard, net, comm, mask="train", weight=weight, ignore_index=IGNORE, reduction=r) for r in ("mean", "sum")}
        res["scores"] = sharded.evaluate(shard, mask="test", ignore_index=IGNORE)
        net.zero_grad()
        empty = sharded.loss(shard, mask="none", weight=weight, ignore_index=IGNORE)
        empty.backward()
        res["empty"] = (float(empty), all(not bool(q.grad.any()) and bool(torch.isfinite(q.grad).all()) for q in net.parameters()))
        return res

    results = pd.run_thread_world(world, body, DEV)
    for r in ("mean", "sum"):
        _assert_against([res[r] for res in results], *want[r], f"{name} world {world} {r}")
    conf = _numpy_confusion(want["mean"][0], prob["y"], prob["masks"]["test"])
    assert int(conf.sum()) > 0
    for res in results:
        assert np.array_equal(res["scores"]["confusion"].cpu().numpy(), conf)
        assert res["scores"]["accuracy"] == pytest.approx(np.trace(conf) / conf.sum(), abs=1e-12)
        assert np.isnan(res["empty"][0]) and res["empty"][1]


# ------------------------------------------------------------------------------------------------------------------ 3. implicit features
def _no_eye(*args, **kwargs):
    raise AssertionError("torch.eye was called: the default one-hot features were materialised")


_IMPLICIT = {}


def _implicit_problem(hidden):
    key = tuple(hidden)
    if key not in _IMPLICIT:
        from oracle import dbgnn as od
        from oracle import model as om
        prob = _IMPLICIT.get("prob") or _stream(21, 1500, 50, 14, 1200, True)
        _IMPLICIT["prob"] = prob
        params = od.init_params(CLASSES, (prob["n"], prob["n_ho"]), hidden, seed=5)
        _IMPLICIT[key] = (prob, params, om.dbgnn_inputs(prob["layers"], 2, "last"))           # (x = x_h = torch.eye: the explicit identity)
    return _IMPLICIT[key]


@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("hidden", [[16, 32, 8], [6, 10, 3]], ids=["fused", "composition"])
@pytest.mark.parametrize("world", [1, 3, 8])
def test_implicit_one_hot_features_on_shards(world, hidden, p, monkeypatch):
    """Shards of ``build_dbgnn_shard(x=None, x_h=None)`` and of ``shard_dbgnn_bundle`` on a default ``to_dbgnn_data`` bundle, ``torch.eye``
    forbidden while they are built and stepped: logits, loss share and every gradient against the float64 reference on an explicit identity
    (with the reference's masks under dropout), and against the single-GPU ``DBGNN`` on the bundle with the same seed."""
    _need_gpu()
    import pathpyg_amd as pp
    import pathpyg_amd.nn.dbgnn as mod
    from pathpyg_amd import distributed as pd
    from pathpyg_amd.nn.sharded import HipOps
    prob, params, inputs = _implicit_problem(hidden)
    n, n_ho = prob["n"], prob["n_ho"]
    tg = _graph(pp, prob)
    y = prob["y"].clamp(min=0).to(DEV)
    mask = prob["masks"]["train"].to(DEV)

    def body(comm):
        res = {}
        for source in ("stream", "bundle"):
            if source == "stream":
                shard = pd.build_dbgnn_shard(tg, prob["delta"], None, None, y, comm, masks={"train": mask})
                key = "train"
            else:
                data = pp.MultiOrderModel.from_temporal_graph(tg, delta=prob["delta"], max_order=2).to_dbgnn_data()
                data.y, data.train_mask = y, mask
                shard = pd.shard_dbgnn_bundle(data, comm)
                assert data.is_identity("x") and data.is_identity("x_h") and data.peek("x").value is None
                key = "train_mask"
            assert shard.x is None and shard.x_h is None and shard.ho.rows.numel() == shard.ho.n_src
            fused = HipOps.one_hot_fused_ok(shard.ho.plan, hidden[0])
            assert fused == (hidden[0] % 4 == 0)
            net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(n, n_ho), hidden_dims=hidden, p_dropout=p).to(DEV)
            net.load_state_dict(params)
            net.train()
            sharded = pd.ShardedDBGNN(net, comm)
            net.zero_grad()
            share = sharded.loss(shard, mask=key)
            seed = sharded.last_seed
            share.backward()
            pd.all_reduce_gradients(net, average=False, comm=comm)
            out = None
            if p == 0:
                out = sharded(shard).detach()
            res[source] = {"out": out, "lo": shard.fo.lo, "hi": shard.fo.hi, "share": share.detach().double().cpu(), "seed": seed,
                           "grads": {k: v.grad.detach().clone() for k, v in net.named_parameters()}}
        return res

    with monkeypatch.context() as patch:
        patch.setattr(torch, "eye", _no_eye)
        results = pd.run_thread_world(world, body, DEV)
    for source in ("stream", "bundle"):
        ranks = [r[source] for r in results]
        seed = ranks[0]["seed"]
        assert all(r["seed"] == seed for r in ranks) and (seed is None) == (p == 0)
        want_out, want_loss, want_grads = _reference(params, inputs, y.cpu(), mask.cpu(), weight=None, ignore_index=None, p=p, seed=seed or 0)
        what = f"{source} world {world} hidden {hidden} p {p}"
        if p == 0:
            _assert_against(ranks, want_out, want_loss, want_grads, what)
        else:
            assert sum(float(r["share"]) for r in ranks) == pytest.approx(float(want_loss), rel=RTOL, abs=ATOL)
            _gradients_close(ranks[0]["grads"], want_grads, what)
        # the single-GPU model on the default bundle, same seed: the same elements are dropped at every site
        data = pp.MultiOrderModel.from_temporal_graph(tg, delta=prob["delta"], max_order=2).to_dbgnn_data()
        net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(n, n_ho), hidden_dims=hidden, p_dropout=p).to(DEV)
        net.load_state_dict(params)
        net.train()
        with monkeypatch.context() as patch:
            patch.setattr(mod, "_draw_seed", lambda: seed)
            loss = pp.nn.cross_entropy(net(data), y, mask=mask)
        loss.backward()
        assert sum(float(r["share"]) for r in ranks) == pytest.approx(float(loss), rel=RTOL, abs=ATOL)
        _gradients_close(ranks[0]["grads"], {name: prm.grad for name, prm in net.named_parameters()}, f"{what} vs single GPU")


def test_implicit_shards_hold_no_feature_rows_and_hub_rows_take_the_composition(monkeypatch):
    """(a) 20 000 events over 2 000 nodes on 3 ranks: a rank's explicit higher-order feature rows would be (n_own + n_halo) x n_ho floats, at
    least n_ho^2 * 4 / 3 bytes (hundreds of MB).  Build + one dropout training step of ALL three ranks together stay under a quarter of ONE
    rank's rows — no tensor with n columns but the parameters, their transposes and gradients can exist.  (b) a star stream whose hub collects
    600 in-neighbours: the first-order plan carries a hub row, the fused kernel is refused, the composition route matches the reference."""
    _need_gpu()
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    from pathpyg_amd.nn.sharded import HipOps
    from oracle import dbgnn as od
    from oracle import model as om
    gen = torch.Generator().manual_seed(4)
    events, nodes = 20_000, 2_000
    tg = pp.TemporalGraph(pp.Data(edge_index=torch.randint(0, nodes, (2, events), generator=gen).to(DEV), time=torch.randperm(events, generator=gen).to(DEV),
                                  num_nodes=nodes))
    y = torch.randint(0, CLASSES, (nodes,), generator=gen).to(DEV)
    mask = (torch.arange(nodes) % 3 != 0).to(DEV)

    def big(comm):
        shard = pd.build_dbgnn_shard(tg, 40, None, None, y, comm, masks={"train": mask})
        net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(nodes, shard.n_ho), hidden_dims=[16, 32, 8], p_dropout=0.4).to(DEV)
        net.train()
        sharded = pd.ShardedDBGNN(net, comm)
        loss = sharded.loss(shard, mask="train")
        loss.backward()
        pd.all_reduce_gradients(net, average=False, comm=comm)
        return shard.n_ho, float(loss), shard.ho.n_src

    with monkeypatch.context() as patch:
        patch.setattr(torch, "eye", _no_eye)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        results = pd.run_thread_world(3, big, DEV)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    n_ho = results[0][0]
    assert n_ho >= 15_000 and np.isfinite(sum(r[1] for r in results))
    one_rank_rows = min(r[2] for r in results) * n_ho * 4
    print(f"[memory] peak {peak / 2 ** 20:.1f} MiB for 3 ranks; one rank's explicit x_h rows alone: {one_rank_rows / 2 ** 20:.1f} MiB")
    assert peak < one_rank_rows / 4
    # ---- (b) hub row
    rng = np.random.default_rng(5)
    n, hub = 700, 650
    src = np.concatenate((np.arange(600), rng.integers(0, n, 900), np.full(300, hub)))
    dst = np.concatenate((np.full(600, hub), rng.integers(0, n, 900), rng.integers(0, n, 300)))
    order = rng.permutation(src.size)
    prob = {"ei": torch.from_numpy(np.stack((src[order], dst[order]))), "t": torch.arange(src.size), "w": None, "n": n, "delta": 3}
    layers = om.layers_from_temporal(prob["ei"], prob["t"], n, delta=3, max_order=2)
    n_ho = layers[2]["num_nodes"]
    hidden = [16, 32, 8]
    params = od.init_params(CLASSES, (n, n_ho), hidden, seed=7)
    yh = torch.randint(0, CLASSES, (n,), generator=gen)
    mh = torch.arange(n) % 2 == 0
    want = _reference(params, om.dbgnn_inputs(layers, 2, "last"), yh, mh, weight=None, ignore_index=None)
    tgh = _graph(pp, prob)

    def hubbed(comm):
        shard = pd.build_dbgnn_shard(tgh, 3, None, None, yh.to(DEV), comm, masks={"m": mh.to(DEV)})
        net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(n, n_ho), hidden_dims=hidden).to(DEV)
        net.load_state_dict(params)
        res = _step(pd, pd.ShardedDBGNN(net, comm), shard, net, comm, mask="m")
        res["hub"] = shard.fo.plan.fwd_heavy is not None and shard.fo.plan.fwd_heavy.n_heavy > 0 and not HipOps.one_hot_fused_ok(shard.fo.plan, 16)
        return res

    ranks = pd.run_thread_world(3, hubbed, DEV)
    assert any(r["hub"] for r in ranks)
    _assert_against(ranks, *want, "hub row")


# ------------------------------------------------------------------------------------------------------------------ 4. the whole loop
def test_training_loop_on_three_ranks_equals_the_single_gpu_loop():
    """5 Adam steps of the README loop — masked loss, gradient all-reduce, ``pp.nn.optim.Adam``, then ``evaluate`` — on 3 emulated ranks with
    implicit features and dropout, against the same loop on one GPU from the same weights and seeds: the loss of every step at the loss bar."""
    _need_gpu()
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as pd
    prob, params, _ = _implicit_problem([16, 32, 8])
    n, n_ho, tg = prob["n"], prob["n_ho"], _graph(pp, prob)
    y = prob["y"].to(DEV)
    seeds = [101, 202, 303, 404, 505]

    def model():
        net = pp.nn.DBGNN(num_classes=CLASSES, num_features=(n, n_ho), hidden_dims=[16, 32, 8], p_dropout=0.4).to(DEV)
        net.load_state_dict(params)
        return net

    # ---- one GPU
    data = pp.MultiOrderModel.from_temporal_graph(tg, delta=prob["delta"], max_order=2).to_dbgnn_data()
    data.y = y
    data.train_mask, data.test_mask = prob["masks"]["train"].to(DEV), prob["masks"]["test"].to(DEV)
    net = model()
    opt = pp.nn.optim.Adam(net.parameters(), lr=1e-2)
    single = []
    for s in seeds:
        net.train()
        opt.zero_grad()
        torch.manual_seed(s)                     # (the forward pass draws its dropout seed from torch's CPU generator)
        loss = pp.nn.cross_entropy(net(data), data.y, mask=data.train_mask, ignore_index=IGNORE)
        loss.backward()
        opt.step()
        single.append(float(loss))
    net.eval()
    single_scores = pp.nn.evaluate(net(data), data.y, mask=data.test_mask, ignore_index=IGNORE)

    # ---- three ranks
    def body(comm):
        rank_net = model()
        sharded = pd.ShardedDBGNN(rank_net, comm)
        shard = sharded.prepare(data)
        rank_opt = pp.nn.optim.Adam(rank_net.parameters(), lr=1e-2)
        shares, drawn = [], []
        for s in seeds:
            rank_net.train()
            rank_opt.zero_grad()
            torch.manual_seed(s)                 # (ranks run one at a time between collectives: each draws the single-GPU step's seed)
            share = sharded.loss(shard, mask="train_mask", ignore_index=IGNORE)
            drawn.append(sharded.last_seed)
            share.backward()
            pd.all_reduce_gradients(rank_net, average=False, comm=comm)
            rank_opt.step()
            shares.append(float(share))
        rank_net.eval()
        return shares, sharded.evaluate(shard, mask="test_mask", ignore_index=IGNORE), drawn

    results = pd.run_thread_world(3, body, DEV)
    for step, want in enumerate(single):
        print(f"[loop] step {step}: single GPU {want:.9g}, 3 ranks {sum(r[0][step] for r in results):.9g}")
    for step, want in enumerate(single):
        assert sum(r[0][step] for r in results) == pytest.approx(want, rel=RTOL, abs=ATOL), f"step {step}"
    assert all(r[2] == results[0][2] for r in results) and len(set(results[0][2])) == len(seeds)
    for _, scores, _ in results:
        assert torch.equal(scores["confusion"].cpu(), single_scores["confusion"].cpu()) and scores["accuracy"] == single_scores["accuracy"]
