"""The DBGNN's default one-hot features stay implicit on the GPU: ``to_dbgnn_data()`` stores a deferred ``Identity``, ``DBGNN.forward`` reads
``W^T`` (eval) or ``diag(d) W^T`` (training with dropout, ``pp_dropout_diag_rows_f32``) through the CSR and no ``n x n`` matrix is ever made.
Bars: those of tests/test_gpu_dbgnn.py for the same comparison (1e-5 relative fp32 with an absolute floor; gradients 1e-4 relative with a floor
of 2e-5 of the largest entry)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-5, 2e-6
P = 0.4


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def _no_eye(*args, **kwargs):
    raise AssertionError("torch.eye was called: the one-hot features must stay implicit")


def _path_model(pp, n=20, walks=200, length=5, seed=0):
    gen = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, n, (walks, length), generator=gen)
    paths = pp.PathData(pp.IndexMap([str(i) for i in range(n)]), device=DEV)
    paths.append_walks([tuple(str(int(v)) for v in row) for row in rows], weights=[1.0] * walks)
    return pp.MultiOrderModel.from_path_data(paths, max_order=2)


def _temporal_model(pp, n=20, events=700, span=2000, delta=40, seed=1, num_nodes=None, extra=()):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, events), generator=gen)
    t = torch.randint(0, span, (events,), generator=gen)
    if extra:
        ei = torch.cat((ei, torch.tensor([[a for a, _, _ in extra], [b for _, b, _ in extra]])), dim=1)
        t = torch.cat((t, torch.tensor([c for _, _, c in extra])))
    g = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=n if num_nodes is None else num_nodes))
    return pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=2)


_MODELS = {}


def _model(pp, kind):
    """One model per kind for the whole module (the bundles are made per test: a bundle is what the tests look at)."""
    if kind not in _MODELS:
        if kind == "paths":
            _MODELS[kind] = _path_model(pp)
        elif kind == "temporal":
            _MODELS[kind] = _temporal_model(pp)
        elif kind == "temporal_isolated":       # node 20 never occurs (isolated: only its GCN self term), node 3 has a self-loop
            _MODELS[kind] = _temporal_model(pp, num_nodes=21, extra=((3, 3, 100), (3, 3, 104), (3, 5, 108)))
        else:
            # two stars.  In-hub: L leaves a_i -> 0, then 0 -> b_j (3 of them): the order-2 nodes (0, b_j) have L in-neighbours (a_i, 0) — hub rows of
            # the FORWARD plans (node 0 in the first-order one).  Out-hub: c_j -> 1 (3), then 1 -> d_i (L): the nodes (c_j, 1) have L out-neighbours
            # — hub rows of the BACKWARD plans.  L exceeds the chunk of the hub pre-pass, so a hub row takes more than one chunk.
            from pathpyg_amd import _hip
            L = max(int(_hip.lib().pp_heavy_chunk_entries()), _hip.HEAVY_ROW_ENTRIES) + 40
            a, b, c, d = (torch.arange(k) + off for k, off in ((L, 2), (3, 2 + L), (3, 5 + L), (L, 8 + L)))
            zero, one = torch.zeros(L, dtype=torch.int64), torch.ones(L, dtype=torch.int64)
            ei = torch.cat((torch.stack((a, zero)), torch.stack((zero[:3], b)), torch.stack((c, one[:3])), torch.stack((one, d))), dim=1)
            t = torch.cat((torch.arange(L), L + 10 + torch.arange(3), torch.arange(3), 10 + torch.arange(L)))
            g = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=2 * L + 8))
            _MODELS[kind] = pp.MultiOrderModel.from_temporal_graph(g, delta=2 * L + 100, max_order=2)
    return _MODELS[kind]


def _unresolved(data):
    from pathpyg_amd.data import Identity
    return all(isinstance(data.peek(k), Identity) and data.peek(k).value is None for k in ("x", "x_h"))


def _cpu_inputs(mom, mapping):
    """The bundle's tensors on the CPU with a REAL identity for x / x_h, from a bundle of its own (the one under test stays unresolved)."""
    ref = mom.to_dbgnn_data(max_order=2, mapping=mapping)
    n, n_ho = int(ref.num_nodes), int(ref.num_ho_nodes)
    names = ("edge_index", "edge_weights", "edge_index_higher_order", "edge_weights_higher_order", "bipartite_edge_index")
    out = {k: getattr(ref, k).cpu() for k in names}
    out.update(num_nodes=n, num_ho_nodes=n_ho, x=torch.eye(n), x_h=torch.eye(n_ho))
    return out


def _net(pp, params, classes, features, hidden, p=0.0):
    net = pp.nn.DBGNN(num_classes=classes, num_features=features, hidden_dims=list(hidden), p_dropout=0.0)
    net.load_state_dict(params, strict=True)
    net.p_dropout = p
    return net.to(DEV)


def _masked_reference(params, cpu, y, hidden, p, seed):
    """The reference forward (dbgnn.py:131-150) on the CPU with the masks of ``dropout_mask`` at every site, on a real identity."""
    from oracle import dbgnn as od
    import pathpyg_amd.nn.dbgnn as mod
    from pathpyg_amd.nn.sharded import dropout_mask
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    drop = lambda t, tag: t * dropout_mask(torch.arange(t.size(0)), t.size(1), p, seed, tag)
    x, x_h = cpu["x"], cpu["x_h"]
    for i in range(len(hidden) - 1):
        x = F.elu(od.gcn_conv(drop(x, mod.TAG_FO + i), cpu["edge_index"], cpu["edge_weights"], leaves[f"first_order_layers.{i}.lin.weight"],
                              leaves[f"first_order_layers.{i}.bias"]))
    x = drop(x, mod.TAG_FO_OUT)
    for i in range(len(hidden) - 1):
        x_h = F.elu(od.gcn_conv(drop(x_h, mod.TAG_HO + i), cpu["edge_index_higher_order"], cpu["edge_weights_higher_order"],
                                leaves[f"higher_order_layers.{i}.lin.weight"], leaves[f"higher_order_layers.{i}.bias"]))
    x_h = drop(x_h, mod.TAG_HO_OUT)
    x = F.elu(od.bipartite_op(x_h, x, cpu["bipartite_edge_index"], cpu["num_nodes"], leaves["bipartite_layer.lin1.weight"],
                              leaves["bipartite_layer.lin1.bias"], leaves["bipartite_layer.lin2.weight"], leaves["bipartite_layer.lin2.bias"]))
    out = drop(x, mod.TAG_HEAD) @ leaves["lin.weight"].t() + leaves["lin.bias"]
    loss = F.cross_entropy(out, y)
    loss.backward()
    return out.detach(), loss.detach(), {k: v.grad for k, v in leaves.items()}


def _assert_step_close(out, loss, net, want_out, want_loss, want_grads):
    scale = float(want_out.abs().max()) + 1e-12
    torch.testing.assert_close(out.detach().cpu(), want_out, rtol=RTOL, atol=max(ATOL, 2e-6 * scale))
    torch.testing.assert_close(loss.detach().cpu(), want_loss, rtol=RTOL, atol=ATOL)
    for name, prm in net.named_parameters():
        gs = float(want_grads[name].abs().max()) + 1e-12
        torch.testing.assert_close(prm.grad.cpu(), want_grads[name], rtol=RTOL * 10, atol=max(ATOL, 2e-5 * gs), msg=lambda s_: f"{name}: {s_}")


def _train_step(net, data, y, seed_of=77):
    import pathpyg_amd.nn.dbgnn as mod
    net.train()
    net.zero_grad()
    torch.manual_seed(seed_of)
    seed = mod._draw_seed()
    torch.manual_seed(seed_of)                  # the model's forward draws the same seed
    out = net(data)
    loss = F.cross_entropy(out, y.to(DEV))
    loss.backward()
    return out, loss, seed


# ------------------------------------------------------------------------------------------------------------------ 3. no identity is ever built
def test_default_features_never_build_an_identity(pp, monkeypatch):
    monkeypatch.setattr(torch, "eye", _no_eye)
    gen = torch.Generator().manual_seed(3)
    for mom in (_path_model(pp, walks=100), _temporal_model(pp, events=300)):
        data = mom.to_dbgnn_data()
        assert _unresolved(data)
        n, n_ho = int(data.num_nodes), int(data.num_ho_nodes)
        assert (n, n_ho) == (mom.layers[1].n, mom.layers[2].n) and data.peek("x_h").shape == (n_ho, n_ho)
        y = torch.randint(0, 2, (n,), generator=gen).to(DEV)
        mask = (torch.arange(n) % 3 != 0).to(DEV)
        torch.manual_seed(5)
        net = pp.nn.DBGNN(num_classes=2, num_features=(n, n_ho), hidden_dims=[16, 32, 8], p_dropout=P).to(DEV)
        net.eval()
        out = net(data)
        assert out.shape == (n, 2) and bool(torch.isfinite(out).all())
        net.train()
        opt = pp.nn.optim.Adam(net.parameters(), lr=1e-2)
        before = net.higher_order_layers[0].lin.weight.detach().clone()
        opt.zero_grad()
        loss = pp.nn.cross_entropy(net(data), y, mask=mask)
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss)) and not torch.equal(net.higher_order_layers[0].lin.weight.detach(), before)
        assert data.to(DEV) is data and _unresolved(data)
        copy = data.clone()
        assert _unresolved(copy) and copy.is_identity("x") and copy.is_identity("x_h")
        net.eval()
        again = net(data)
        torch.testing.assert_close(net(copy), again, rtol=RTOL, atol=ATOL)   # (the copy builds plans of its own from copies of the tensors)
        assert net(data.to(DEV)).shape == (n, 2)
        assert _unresolved(data) and _unresolved(copy)


# ------------------------------------------------------------------------------------------------------------------ 4. size
def test_default_features_at_a_size_where_the_identity_would_not_fit_the_cap(pp, monkeypatch):
    """20 000 events over 2 000 nodes: ``n_ho`` is near 20 000, the identity alone would be ``n_ho^2 * 4`` bytes (1.6 GB); bundle + one dropout
    training step must stay under half of that (its own tensors are a few tens of MB)."""
    monkeypatch.setattr(torch, "eye", _no_eye)
    gen = torch.Generator().manual_seed(4)
    events, nodes = 20_000, 2_000
    ei = torch.randint(0, nodes, (2, events), generator=gen)
    t = torch.randperm(events, generator=gen)                               # distinct timestamps
    g = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=nodes))
    mom = pp.MultiOrderModel.from_temporal_graph(g, delta=40, max_order=2)
    n, n_ho = mom.layers[1].n, mom.layers[2].n
    assert n == nodes and n_ho >= 15_000
    y = torch.randint(0, 3, (n,), generator=gen).to(DEV)
    mask = (torch.arange(n) % 2 == 0).to(DEV)
    torch.manual_seed(6)
    net = pp.nn.DBGNN(num_classes=3, num_features=(n, n_ho), hidden_dims=[16, 32, 8], p_dropout=P).to(DEV)
    opt = pp.nn.optim.Adam(net.parameters(), lr=1e-2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    data = mom.to_dbgnn_data()
    net.train()
    opt.zero_grad()
    loss = pp.nn.cross_entropy(net(data), y, mask=mask)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"n_ho = {n_ho}: peak growth {grown / 2 ** 20:.1f} MiB, cap {n_ho * n_ho * 4 / 2 / 2 ** 20:.1f} MiB")
    assert bool(torch.isfinite(loss)) and _unresolved(data)
    assert grown < n_ho * n_ho * 4 / 2, (grown, n_ho)


# ------------------------------------------------------------------------------------------------------------------ 5. the row-scale kernel
@pytest.mark.parametrize("n_rows,f,n,row0", [(1, 4, 1, 0), (65, 16, 65, 0), (4097, 64, 4097, 0), (300, 8, 1000, 700), (70_001, 16, 70_001, 0),
                                             (129, 6, 200, 50), (33, 300, 33, 0)])      # + widths off the 16-byte path and beyond 256
@pytest.mark.parametrize("p", [0.4, 0.0])
def test_row_scale_kernel_equals_the_torch_statement_bit_for_bit(pp, n_rows, f, n, row0, p):
    from pathpyg_amd import _hip
    from pathpyg_amd.nn.sharded import dropout_mask_diagonal
    seed, tag = 987654321, 64
    x = torch.randn(n_rows, f, generator=torch.Generator().manual_seed(n_rows + f))
    d = dropout_mask_diagonal(torch.arange(row0, row0 + n_rows), n, p, seed, tag)
    want = x * d.unsqueeze(1)                       # (exact: the factor is 0 or 1 / (1 - p), one rounding at most, the same one)
    if p == 0.0:
        assert torch.equal(want, x)
    elif n_rows >= 65:
        assert 0 < int((d == 0).sum()) < n_rows
    gx = x.to(DEV)
    got = _hip.dropout_diag_rows(gx, n, p, seed, tag, row0)
    assert got.data_ptr() != gx.data_ptr() and torch.equal(gx.cpu(), x)
    assert torch.equal(got.cpu(), want)
    same = _hip.dropout_diag_rows(gx, n, p, seed, tag, row0, out=gx)         # out aliases x
    assert same is gx and torch.equal(gx.cpu(), want)


def test_row_scale_kernel_refuses_rows_outside_the_identity(pp):
    from pathpyg_amd import _hip
    x = torch.ones(10, 4, device=DEV)
    with pytest.raises(ValueError):
        _hip.dropout_diag_rows(x, 12, P, 1, 0, row0=3)                       # rows 3 .. 13 of a 12 x 12 identity
    with pytest.raises(ValueError):
        _hip.dropout_diag_rows(x, 12, 1.0, 1, 0)


# ------------------------------------------------------------------------------------------------------------------ 6. training parity
@pytest.mark.parametrize("kind", ["paths", "temporal", "temporal_isolated"])
@pytest.mark.parametrize("mapping", ["last", "both"])
@pytest.mark.parametrize("hidden", [[16, 32, 8], [6, 10, 3]])
def test_dropout_training_on_default_features_matches_masked_reference(pp, kind, mapping, hidden):
    """Logits, loss and every gradient of one training step with p_dropout = 0.4 on the DEFAULT bundle against a torch-CPU evaluation of the
    reference forward on a real identity with the same masks; the columns of the first layers' weights whose one-hot row was dropped get a
    gradient of exactly zero."""
    from oracle import dbgnn as od
    from pathpyg_amd.nn.sharded import dropout_mask_diagonal
    import pathpyg_amd.nn.dbgnn as mod
    mom = _model(pp, kind)
    cpu = _cpu_inputs(mom, mapping)
    n, n_ho = cpu["num_nodes"], cpu["num_ho_nodes"]
    assert n == (21 if kind == "temporal_isolated" else 20) and 300 <= n_ho <= 400, (n, n_ho)
    if kind == "temporal_isolated":
        ei = cpu["edge_index"]
        assert int((ei == 20).sum()) == 0 and bool(((ei[0] == 3) & (ei[1] == 3)).any())
    y = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(9))
    params = od.init_params(3, (n, n_ho), hidden, seed=2)
    net = _net(pp, params, 3, (n, n_ho), hidden, P)
    data = mom.to_dbgnn_data(max_order=2, mapping=mapping)
    out, loss, seed = _train_step(net, data, y)
    assert _unresolved(data)
    _assert_step_close(out, loss, net, *_masked_reference(params, cpu, y, hidden, P, seed))
    for stack, tag, size in (("first_order_layers", mod.TAG_FO, n), ("higher_order_layers", mod.TAG_HO, n_ho)):
        dropped = dropout_mask_diagonal(torch.arange(size), size, P, seed, tag) == 0
        grad = getattr(net, stack)[0].lin.weight.grad.cpu()
        assert bool(dropped.any()) and not bool(dropped.all())
        assert bool((grad[:, dropped] == 0).all()) and bool((grad[:, ~dropped] != 0).any()), stack


# ------------------------------------------------------------------------------------------------------------------ 7. the dense route
@pytest.mark.parametrize("kind,mapping,hidden", [("paths", "last", [16, 32, 8]), ("temporal", "last", [16, 32, 8]), ("temporal", "both", [6, 10, 3])])
def test_default_features_give_the_numbers_of_an_explicit_identity(pp, kind, mapping, hidden):
    """The same model and seed on the default bundle and on ``x = torch.eye(n)``, ``x_h = torch.eye(n_ho)`` passed explicitly (the dense route:
    dropout of the n x n matrix, then the layer kernels): same logits and gradients in training with dropout, same outputs in eval mode."""
    from oracle import dbgnn as od
    mom = _model(pp, kind)
    n, n_ho = mom.layers[1].n, mom.layers[2].n
    y = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(10))
    params = od.init_params(3, (n, n_ho), hidden, seed=4)
    results = []
    for explicit in (False, True):
        feats = dict(x=torch.eye(n, device=DEV), x_h=torch.eye(n_ho, device=DEV)) if explicit else {}
        data = mom.to_dbgnn_data(max_order=2, mapping=mapping, **feats)
        assert data.is_identity("x") != explicit and data.is_identity("x_h") != explicit
        net = _net(pp, params, 3, (n, n_ho), hidden, P)
        out, loss, _ = _train_step(net, data, y)
        net.eval()
        quiet = _net(pp, params, 3, (n, n_ho), hidden, 0.0).train()
        results.append((out.detach().cpu(), loss.detach().cpu(), {k: v.grad.cpu() for k, v in net.named_parameters()},
                        net(data).detach().cpu(), quiet(data).detach().cpu()))
    (out_a, loss_a, grads_a, eval_a, quiet_a), (out_b, loss_b, grads_b, eval_b, quiet_b) = results
    scale = float(out_b.abs().max()) + 1e-12
    torch.testing.assert_close(out_a, out_b, rtol=RTOL, atol=max(ATOL, 2e-6 * scale))
    torch.testing.assert_close(loss_a, loss_b, rtol=RTOL, atol=ATOL)
    for name in grads_b:
        gs = float(grads_b[name].abs().max()) + 1e-12
        torch.testing.assert_close(grads_a[name], grads_b[name], rtol=RTOL * 10, atol=max(ATOL, 2e-5 * gs), msg=lambda s_: f"{name}: {s_}")
    scale = float(eval_b.abs().max()) + 1e-12
    torch.testing.assert_close(eval_a, eval_b, rtol=RTOL, atol=max(ATOL, 2e-6 * scale))
    torch.testing.assert_close(quiet_a, quiet_b, rtol=RTOL, atol=max(ATOL, 2e-6 * scale))
    torch.testing.assert_close(quiet_a, eval_a, rtol=0, atol=0)            # p_dropout == 0 in training mode is the eval route


# ------------------------------------------------------------------------------------------------------------------ 8. no n x n operand
def test_dropout_training_step_on_default_features_launches_no_gemm_and_no_eye(pp):
    from oracle import dbgnn as od
    mom = _model(pp, "paths")
    n, n_ho = mom.layers[1].n, mom.layers[2].n
    y = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(11))
    net = _net(pp, od.init_params(3, (n, n_ho), [16, 32, 8], seed=5), 3, (n, n_ho), [16, 32, 8], P)
    data = mom.to_dbgnn_data()
    _train_step(net, data, y)                                               # plans are built outside the profile
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
        _train_step(net, data, y)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert not [k for k in names if "Cijk" in k or "gemm" in k.lower() or "addmm" in k.lower() or "aten::mm" in k or "aten::eye" in k], names
    assert not [k for k in names if "k_dropout_diag_rows" in k], names        # no scaled copy of W^T either: the factor rides in the aggregation
    assert _unresolved(data)


# ------------------------------------------------------------------------------------------------------------------ the two routes of the first layer
def test_plans_with_hub_rows_take_the_row_scale_route(pp):
    """A higher-order (and first-order) plan with hub rows in both directions: the fused first layer does not take them (the chunked hub
    pre-pass sums unscaled rows), the row-scale route does — same numbers as the masked reference."""
    from oracle import dbgnn as od
    import pathpyg_amd.nn.dbgnn as mod
    mom = _model(pp, "stars")
    cpu = _cpu_inputs(mom, "last")
    n, n_ho = cpu["num_nodes"], cpu["num_ho_nodes"]
    data = mom.to_dbgnn_data()
    plan_fo, plan_ho, _ = mod._valid_plans(data)
    assert plan_ho.fwd_heavy is not None and plan_ho.bwd_heavy is not None and plan_fo.fwd_heavy is not None
    assert plan_ho.fwd_heavy.n_chunks > plan_ho.fwd_heavy.n_heavy                  # a hub row of more than one chunk
    assert not mod._OneHotDropLayer.supported(plan_ho, 16) and not mod._OneHotDropLayer.supported(plan_fo, 16)
    y = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(13))
    params = od.init_params(3, (n, n_ho), [16, 32, 8], seed=7)
    net = _net(pp, params, 3, (n, n_ho), [16, 32, 8], P)
    out, loss, seed = _train_step(net, data, y)
    _assert_step_close(out, loss, net, *_masked_reference(params, cpu, y, [16, 32, 8], P, seed))
    assert _unresolved(data)


@pytest.mark.parametrize("n,e,f", [(1, 1, 4), (65, 300, 16), (4097, 30_000, 64), (300, 9000, 100), (1000, 5000, 256), (70_001, 200_000, 8)])
@pytest.mark.parametrize("p", [0.4, 0.0])
def test_fused_aggregation_with_the_diagonal_factor_equals_the_row_scale_composition(pp, n, e, f, p):
    """pp_spmm_diag_drop_f32 against pp_dropout_diag_rows_f32 around pp_spmm_f32: the factor on the source rows (forward, with bias and ELU) and on
    the output rows (backward).  Forward the two differ by the rounding of ``(v * d) * x`` against ``v * (x * d)`` (the bar of the aggregation
    kernels' own tests: 1e-5 relative, 2e-6 of the largest value absolute); backward it is the same sum and one more product, and rows whose
    factor is 0 are exactly 0."""
    from pathpyg_amd import _hip
    g = torch.Generator().manual_seed(n + e + f)
    row = torch.sort(torch.randint(0, n, (e,), generator=g)).values
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0).int()
    idx = torch.randint(0, n, (e,), generator=g, dtype=torch.int32)
    val, sc = torch.rand(e, generator=g), torch.rand(n, generator=g)
    x, bias = torch.randn(n, f, generator=g), torch.randn(f, generator=g)
    ptr, idx, val, sc, x, bias = (t.to(DEV) for t in (ptr, idx, val, sc, x, bias))
    site = (n, p, 24680, 64)
    want = _hip.spmm(ptr, idx, val, n, _hip.dropout_diag_rows(x, *site), sc, None, bias, True)
    got = _hip.spmm_diag_drop(ptr, idx, val, n, x, sc, bias, True, 1, *site)
    torch.testing.assert_close(got, want, rtol=RTOL, atol=2e-6 * float(want.abs().max()))
    lin = _hip.spmm(ptr, idx, val, n, x, sc, x)
    want = _hip.dropout_diag_rows(lin, *site)
    got = _hip.spmm_diag_drop(ptr, idx, val, n, x, sc, None, False, 2, *site)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    dropped = _hip.dropout_diag_rows(torch.ones(n, 4, device=DEV), *site)[:, 0] == 0
    assert bool((got[dropped] == 0).all()) and (p > 0 or not bool(dropped.any()))
