"""pp_dbgnn_head_forward_f32 / pp_dbgnn_head_backward_f32: everything between the bipartite sum and the bipartite backward in one kernel
each way,

    z      = ELU( agg W1^T + deg * (x W2^T + b2 + b1) )          agg [n, Ha], x [n, Hx] (a stored ELU activation), deg [n]
    logits = z Wlin^T + blin                                     [n, C]

checked against a float64 evaluation of these formulas and of their gradients written out below, against the chain of kernels it
replaces (``nn.dbgnn.FUSE_HEAD`` off), and at model level through ``DBGNN`` and ``ShardedDBGNN`` on a stream-built model against the
oracle.  Tolerance: tests/tolerance.py at its default 1e-5; at the largest n a weight gradient that needs more is held to twice what
the chain of kernels needs on the same inputs (both are fp32 sums of the same terms in another order)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.tolerance import assert_embeddings_close, assert_gradients_close, gradient_rtol_needed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# a single row; tail tiles on either side of 16; one full tile group (a workgroup's 4 waves); many workgroups with n = 1 mod 16; more tiles
# than one pass of the resident grid (512 workgroups x 4 waves x 16 rows = 32768)
ROWS = [1, 15, 16, 17, 64, 4097, 70_001]
WIDTHS = [(64, 64, 64), (16, 32, 64), (32, 16, 16)]          # (Ha, Hx, Hb)
CLASSES = [2, 8, 16]
WEIGHT_GRADS = ("dW1", "dW2", "db1", "db2", "dWlin", "dblin", "colsum_fo")


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


def _inputs(n, ha, hx, hb, c):
    g = torch.Generator().manual_seed(1000 * n + 100 * ha + 10 * hx + hb + c)
    deg = torch.randint(0, 41, (n,), generator=g).float()
    deg[::3] = 0.0                                                     # rows without a higher-order neighbour
    if n > 1:
        deg[1] = 40.0
    t = {
        "agg": torch.randn(n, ha, generator=g) * deg.clamp(min=1).sqrt().unsqueeze(1),
        "x": F.elu(torch.randn(n, hx, generator=g)),                 # an ELU output: both signs, never below -1
        "deg": deg,
        "w1": torch.randn(hb, ha, generator=g) / ha ** 0.5, "b1": torch.randn(hb, generator=g) * 0.1,
        "w2": torch.randn(hb, hx, generator=g) / hx ** 0.5, "b2": torch.randn(hb, generator=g) * 0.1,
        "wlin": torch.randn(c, hb, generator=g) / hb ** 0.5, "blin": torch.randn(c, generator=g) * 0.1,
        "dlogits": torch.randn(n, c, generator=g),
    }
    assert bool((t["x"] > 0).any()) or n < 4
    return t


def _float64(t):
    """The formulas of the module docstring and their gradients for a given ``dlogits``, in float64."""
    d = {k: v.double() for k, v in t.items()}
    pre = d["agg"] @ d["w1"].t() + d["deg"].unsqueeze(1) * (d["x"] @ d["w2"].t() + d["b2"] + d["b1"])
    z = torch.where(pre > 0, pre, torch.expm1(pre))
    logits = z @ d["wlin"].t() + d["blin"]
    dz = d["dlogits"] @ d["wlin"]
    dpre = dz * torch.where(z > 0, torch.ones_like(z), z + 1)
    dper = d["deg"].unsqueeze(1) * dpre
    dpre_fo = (dper @ d["w2"]) * torch.where(d["x"] > 0, torch.ones_like(d["x"]), d["x"] + 1)
    return {"z": z, "logits": logits, "d_agg": dpre @ d["w1"], "dpre_fo": dpre_fo, "colsum_fo": dpre_fo.sum(0),
            "dW1": dpre.t() @ d["agg"], "dW2": dper.t() @ d["x"], "db1": dper.sum(0), "db2": dper.sum(0),
            "dWlin": d["dlogits"].t() @ z, "dblin": d["dlogits"].sum(0)}


def _layers(t):
    """``(bipartite layer, lin)`` stand-ins holding the case's weights (``nn.dbgnn.head`` reads ``lin1`` / ``lin2`` only)."""
    def linear(w, b):
        lin = torch.nn.Linear(w.size(1), w.size(0)).to(DEV)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        return lin
    return types.SimpleNamespace(lin1=linear(t["w1"], t["b1"]), lin2=linear(t["w2"], t["b2"])), linear(t["wlin"], t["blin"])


def _through_head(t, fuse, monkeypatch):
    """One forward + backward through ``nn.dbgnn.head`` with ``FUSE_HEAD = fuse``: the results under the names of :func:`_float64` (no z)."""
    from pathpyg_amd.nn import dbgnn
    bl, lin = _layers(t)
    agg, x = t["agg"].to(DEV).requires_grad_(), t["x"].to(DEV).requires_grad_()
    act_bias = torch.zeros(x.size(1), device=DEV, requires_grad=True)
    with monkeypatch.context() as patch:
        patch.setattr(dbgnn, "FUSE_HEAD", fuse)
        logits = dbgnn.head(agg, x, t["deg"].to(DEV), bl, lin, act_bias)
        logits.backward(t["dlogits"].to(DEV))
    return {"logits": logits.detach(), "d_agg": agg.grad, "dpre_fo": x.grad, "colsum_fo": act_bias.grad, "dW1": bl.lin1.weight.grad,
            "dW2": bl.lin2.weight.grad, "db1": bl.lin1.bias.grad, "db2": bl.lin2.bias.grad, "dWlin": lin.weight.grad, "dblin": lin.bias.grad}


def _chain_backward(t, z_in):
    """The backward kernels of the chain (``FUSE_HEAD`` off) on the same stored ``z``: classifier, combine, lin1 and lin2 one after the other."""
    from pathpyg_amd import _hip
    from pathpyg_amd.nn import dbgnn
    bl, lin = _layers(t)
    z = z_in.clone().requires_grad_()
    dbgnn.dense(z, lin).backward(t["dlogits"].to(DEV))
    da, dp, db1 = _hip.bip_combine_backward(z.grad, z_in, t["deg"].to(DEV), True)
    agg, x = t["agg"].to(DEV).requires_grad_(), t["x"].to(DEV).requires_grad_()
    act_bias = torch.zeros(x.size(1), device=DEV, requires_grad=True)
    dbgnn.dense_w(agg, bl.lin1.weight).backward(da)
    dbgnn.dense(x, bl.lin2, True, act_bias).backward(dp)
    return {"d_agg": agg.grad, "dpre_fo": x.grad, "colsum_fo": act_bias.grad, "dW1": bl.lin1.weight.grad, "dW2": bl.lin2.weight.grad, "db1": db1,
            "db2": bl.lin2.bias.grad, "dWlin": lin.weight.grad, "dblin": lin.bias.grad}


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("n", ROWS)
def test_head_kernels_match_float64(pp, n, widths, c):
    from pathpyg_amd import _hip
    ha, hx, hb = widths
    assert _hip.head_supported(ha, hx, hb, c)
    t = _inputs(n, ha, hx, hb, c)
    want = _float64(t)
    assert n < 16 or (bool((want["z"] > 0).any()) and bool((want["z"] < 0).any()))
    d = {k: v.to(DEV) for k, v in t.items()}
    z, logits = _hip.head_forward(d["agg"], d["x"], d["deg"], d["w1"], d["b1"], d["w2"], d["b2"], d["wlin"], d["blin"])
    assert_embeddings_close(z, want["z"], what="z")
    assert_embeddings_close(logits, want["logits"], what="logits")
    # the backward kernel is a function of the STORED z: it gets the float64 z rounded to fp32, so that it is held to its own arithmetic.
    # (ELU'(pre) = z + 1 = exp(pre) on the negative side: its relative error is the ABSOLUTE error of pre, which at deg = 40 is several
    # 1e-5 for any fp32 forward pass, this kernel and the chain alike; the forward error is what the z check above bounds)
    names = ("d_agg", "dpre_fo", "colsum_fo", "dW1", "dW2", "db1", "db2", "dWlin", "dblin")
    z_in = want["z"].float().to(DEV)
    got = dict(zip(names, _hip.head_backward(d["dlogits"], z_in, d["agg"], d["x"], d["deg"], d["w1"], d["w2"], d["wlin"], True)))
    assert_embeddings_close(got["d_agg"], want["d_agg"], what="d_agg")
    assert_embeddings_close(got["dpre_fo"], want["dpre_fo"], what="dpre_fo")
    chain = None
    for name in WEIGHT_GRADS:
        need = gradient_rtol_needed(got[name], want[name])
        print(f"[head n={n} {ha}/{hx}/{hb} C={c}] {name}: fused kernels need rtol {need:.2e}")
        if need <= 1e-5 or n != max(ROWS):
            assert_gradients_close(got[name], want[name], name)
            continue
        # a sum of 7 * 10^4 fp32 terms beyond 1e-5 (the case tests/tolerance.py describes): the chain of kernels on the same inputs sets the bar
        chain = chain if chain is not None else _chain_backward(t, z_in)
        need_chain = gradient_rtol_needed(chain[name], want[name])
        print(f"[head n={n} {ha}/{hx}/{hb} C={c}] {name}: chain of kernels needs rtol {need_chain:.2e}")
        assert need <= 2 * need_chain, f"{name}: fused kernels need rtol {need:.2e}, the chain {need_chain:.2e}"


def test_unsupported_shape_goes_down_the_chain(pp, monkeypatch):
    """Width 48 and 17 classes: no fused variant.  ``head`` gives the chain's result with the flag on, the raw wrappers refuse."""
    from pathpyg_amd import _hip
    t = _inputs(333, 48, 48, 48, 17)
    assert not _hip.head_supported(48, 48, 48, 17) and not _hip.head_supported(64, 64, 48, 8) and not _hip.head_supported(64, 64, 64, 17)
    calls = []
    real = _hip.head_forward
    monkeypatch.setattr(_hip, "head_forward", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    on, off = _through_head(t, True, monkeypatch), _through_head(t, False, monkeypatch)
    assert calls == []
    want = _float64(t)
    for name in on:
        if name in ("logits", "d_agg", "dpre_fo"):            # the same kernels both times (the bias column sums are folded by float atomics)
            assert torch.equal(on[name], off[name]), name
        assert_gradients_close(on[name], want[name], name)
    d = {k: v.to(DEV) for k, v in t.items()}
    with pytest.raises(ValueError):
        real(d["agg"], d["x"], d["deg"], d["w1"], d["b1"], d["w2"], d["b2"], d["wlin"], d["blin"])
    with pytest.raises(ValueError):
        _hip.head_backward(d["dlogits"], torch.zeros(333, 48, device=DEV), d["agg"], d["x"], d["deg"], d["w1"], d["w2"], d["wlin"], True)


def test_head_of_no_rows(pp):
    from pathpyg_amd import _hip
    t = {k: v.to(DEV) for k, v in _inputs(0, 64, 64, 64, 8).items()}
    z, logits = _hip.head_forward(t["agg"], t["x"], t["deg"], t["w1"], t["b1"], t["w2"], t["b2"], t["wlin"], t["blin"])
    assert tuple(z.shape) == (0, 64) and tuple(logits.shape) == (0, 8)
    out = _hip.head_backward(t["dlogits"], z, t["agg"], t["x"], t["deg"], t["w1"], t["w2"], t["wlin"], True)
    assert all(not o.any() for o in out)


# ---------------------------------------------------------------------------------------------------------------- model level
N_FO, DELTA = 300, 120
HIDDEN = {"64": [64, 64, 64], "32-16": [32, 32, 16]}


def _model_case(kind):
    """A small event stream, its order-2 model from the oracle, features, labels, parameters and the oracle's step — computed once."""
    if kind not in _model_case.cache:
        from oracle import dbgnn as od
        from oracle import model as om
        rng = np.random.default_rng(41)
        ei = torch.from_numpy(rng.integers(0, N_FO, (2, 6000)))
        time = torch.from_numpy(np.sort(rng.integers(0, 4000, 6000)))
        sei, st, _ = om.stable_time_sort(ei, time)
        layers = om.layers_from_temporal(sei, st, N_FO, delta=DELTA, max_order=2, edge_weight=None)
        hidden = HIDDEN[kind]
        f = hidden[0]
        gen = torch.Generator().manual_seed(3)
        x, x_h = torch.randn(N_FO, f, generator=gen), torch.randn(layers[2]["num_nodes"], f, generator=gen)
        y = torch.randint(0, 4, (N_FO,), generator=gen)
        params = od.init_params(4, (f, f), hidden, seed=1)
        want = od.loss_and_grads(params, om.dbgnn_inputs(layers, 2, "last", x=x, x_h=x_h), y)
        _model_case.cache[kind] = (ei, time, x, x_h, y, params, hidden, want)
    return _model_case.cache[kind]


_model_case.cache = {}


def _model_step(pp, kind, sharded, fuse, monkeypatch):
    """(logits, loss, {name: grad}, calls of the fused forward) of one step of ``DBGNN`` on the stream's bundle or of ``ShardedDBGNN`` (world 1)
    on the stream's shard."""
    from pathpyg_amd import _hip, distributed as pd
    from pathpyg_amd.nn import dbgnn
    ei, time, x, x_h, y, params, hidden, _ = _model_case(kind)
    g = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=time.to(DEV), num_nodes=N_FO))
    net = pp.nn.DBGNN(num_classes=4, num_features=(hidden[0], hidden[0]), hidden_dims=hidden).to(DEV)
    net.load_state_dict(params)
    calls = []
    real_fwd, real_bwd = _hip.head_forward, _hip.head_backward
    with monkeypatch.context() as patch:
        patch.setattr(dbgnn, "FUSE_HEAD", fuse)
        patch.setattr(_hip, "head_forward", lambda *a, **kw: calls.append("fwd") or real_fwd(*a, **kw))
        patch.setattr(_hip, "head_backward", lambda *a, **kw: calls.append("bwd") or real_bwd(*a, **kw))
        if sharded:
            comm = pd.Comm()
            shard = pd.build_dbgnn_shard(g, DELTA, x.to(DEV), x_h.to(DEV), y.to(DEV), comm)
            model = pd.ShardedDBGNN(net, comm)
            out = model(shard).detach().clone()
            calls.clear()
            loss = model.loss(shard)
        else:
            mom = pp.MultiOrderModel.from_temporal_graph(g, delta=DELTA, max_order=2)
            data = mom.to_dbgnn_data(max_order=2, mapping="last", x=x.to(DEV), x_h=x_h.to(DEV))
            out = net(data)
            loss = pp.nn.cross_entropy(out, y.to(DEV))
            out = out.detach().clone()
        loss.backward()
    return out, loss.detach().clone(), {name: p.grad.clone() for name, p in net.named_parameters()}, calls


@pytest.mark.parametrize("kind", list(HIDDEN))
@pytest.mark.parametrize("sharded", [False, True], ids=["DBGNN", "ShardedDBGNN"])
def test_models_keep_their_results_with_the_fused_head(pp, monkeypatch, sharded, kind):
    """Flag on against flag off and both against the oracle: logits, loss and every parameter gradient."""
    want_out, want_loss, want_grads = _model_case(kind)[7]
    out_off, loss_off, grads_off, calls_off = _model_step(pp, kind, sharded, False, monkeypatch)
    out_on, loss_on, grads_on, calls_on = _model_step(pp, kind, sharded, True, monkeypatch)
    assert calls_off == [] and calls_on == ["fwd", "bwd"]
    for what, out, loss in (("flag on", out_on, loss_on), ("flag off", out_off, loss_off)):
        assert_embeddings_close(out, want_out, what=f"{what} vs the oracle, logits")
        torch.testing.assert_close(loss.cpu(), want_loss, rtol=1e-5, atol=2e-6, msg=lambda s, w=what: f"{w} vs the oracle, loss: {s}")
    assert_embeddings_close(out_on, out_off, what="flag on vs flag off, logits")
    torch.testing.assert_close(loss_on, loss_off, rtol=1e-5, atol=2e-6)
    for name in want_grads:
        print(f"[gradient] {name}: on vs oracle needs rtol {gradient_rtol_needed(grads_on[name], want_grads[name]):.2e}, "
              f"on vs off {gradient_rtol_needed(grads_on[name], grads_off[name]):.2e}")
    for name in want_grads:
        assert_gradients_close(grads_on[name], want_grads[name], f"flag on vs the oracle, {name}")
        assert_gradients_close(grads_off[name], want_grads[name], f"flag off vs the oracle, {name}")
        assert_gradients_close(grads_on[name], grads_off[name], f"flag on vs flag off, {name}")
