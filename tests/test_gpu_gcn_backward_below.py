"""pp_gcn_backward_below_f32: the backward kernel of a stack's second 64 x 64 GCN layer that also forms the FIRST layer's weight gradient
``dW_below = d_in^T (A x)`` from the ``d_in`` tile it holds in registers and never stores ``d_in``.  Checked against float64, against the
two-kernel path it replaces (gcn_backward + weight_grad), for its argument checks, and at model level through ``ShardedDBGNN`` with
``nn.sharded.FUSE_FIRST_DW`` on and off."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.tolerance import assert_gradients_close, gradient_rtol_needed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-5, 2e-6

# (n, e, weighted): a single row without an edge; a tail tile of one row; one full workgroup of self terms; a quarter of the edges in one
# row (the loops over more than 4 and more than 16 neighbours, nnz <= 8 n); many workgroups with n = 1 mod 16 (partial fold + reduce); more
# tiles than one pass of the resident grid; unit values (val = None)
SHAPES = [(1, 0, True), (17, 40, True), (64, 0, True), (300, 2000, True), (4097, 9000, True), (70_001, 200_000, True), (300, 2000, False)]


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


@functools.lru_cache(maxsize=None)
def _case(n, e, weighted):
    """Inputs drawn as in tests/test_gpu_dbgnn.py::test_fused_gcn_backward_kernel (+ agg) and their float64 results, computed once."""
    m = k = 64
    g = torch.Generator().manual_seed(n + e + m + k)
    row = torch.sort(torch.randint(0, n, (e,), generator=g)).values
    if n > 10 and e > 100:
        row[: min(e // 4, 2000)] = row[min(e // 4, 2000)]
        row = torch.sort(row).values
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0).int()
    idx = torch.randint(0, n, (max(e, 1),), generator=g, dtype=torch.int32)[:e]
    val = torch.rand(e, generator=g) if weighted else None
    self_coef = torch.rand(n, generator=g)
    dpre = torch.randn(n, m, generator=g)
    x = F.elu(torch.randn(n, k, generator=g))
    w = torch.randn(m, k, generator=g) / m ** 0.5
    agg = torch.randn(n, 64, generator=g)
    assert e <= 8 * n                                                 # the short-row rule of the variant's caller
    v64 = val.double() if weighted else torch.ones(e, dtype=torch.float64)
    gmat = self_coef.double().unsqueeze(1) * dpre.double()
    gmat.index_add_(0, row, v64.unsqueeze(1) * dpre.double()[idx.long()])
    d = (gmat @ w.double()) * torch.where(x > 0, torch.ones_like(x), x + 1).double()
    want = {
        "colsum": d.sum(0), "colsum_scale": float(d.abs().sum(0).max() + 1),
        "dw": gmat.t() @ x.double(), "dw_scale": float((gmat.abs().t() @ x.double().abs()).max()) + 1e-12,
        "dw_below": d.t() @ agg.double(), "dw_below_scale": float((d.abs().t() @ agg.double().abs()).max()) + 1e-12,
    }
    dev = lambda t_: None if t_ is None else t_.to(DEV)
    return {"n": n, "args": (dev(ptr), dev(idx), dev(val), n, dev(dpre), dev(self_coef), dev(x), dev(w)), "agg": dev(agg), "want": want}


def _assert_matches(got, want, what):
    colsum, dw, dw_below = got
    for name, t, ref, atol in (("colsum", colsum, want["colsum"], 1e-5 * want["colsum_scale"]), ("dW", dw, want["dw"], 2e-6 * want["dw_scale"]),
                               ("dW_below", dw_below, want["dw_below"], 2e-6 * want["dw_below_scale"])):
        err = float((t.double().cpu() - ref.double().cpu()).abs().max())
        print(f"[{what}] {name}: max abs err {err:.3e} (atol {atol:.3e})")
        torch.testing.assert_close(t.cpu(), ref.float().cpu(), rtol=1e-4, atol=atol, msg=lambda s, nm=name: f"{what} {nm}: {s}")


@pytest.mark.parametrize("n,e,weighted", SHAPES)
def test_backward_below_kernel_matches_float64(pp, n, e, weighted):
    """G = A dpre + self * dpre, d = (G W) * ELU'(x); colsum = column sums of d, dW = G^T x, dW_below = d^T agg."""
    from pathpyg_amd import _hip
    c = _case(n, e, weighted)
    _assert_matches(_hip.gcn_backward_below(*c["args"], c["agg"]), c["want"], "float64")


@pytest.mark.parametrize("n,e,weighted", SHAPES)
def test_backward_below_kernel_matches_the_two_kernel_path(pp, n, e, weighted):
    """gcn_backward (d_in stored) + weight_grad(d_in, agg) on the same inputs: results stay what they were."""
    from pathpyg_amd import _hip
    c = _case(n, e, weighted)
    d_in, colsum, dw = _hip.gcn_backward(*c["args"], True, True)
    dw_below = _hip.weight_grad(d_in, c["agg"], want_bias=False)[0]
    # the same float64-derived absolute bounds, with the two-kernel results as the expected values
    want = dict(c["want"], colsum=colsum, dw=dw, dw_below=dw_below)
    _assert_matches(_hip.gcn_backward_below(*c["args"], c["agg"]), want, "two-kernel path")


def test_backward_below_of_an_empty_graph_zeroes_both_gradients(pp):
    from pathpyg_amd import _hip
    z = lambda *s: torch.zeros(*s, device=DEV)
    colsum, dw, dw_below = _hip.gcn_backward_below(torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, 0,
                                                   z(0, 64), z(0), z(0, 64), torch.randn(64, 64, device=DEV), z(0, 64))
    assert not colsum.any() and not dw.any() and not dw_below.any()


def _raw_call(m=64, k=64, k_below=64, fuse_act=1, heavy=False, drop_p=0.0, n_self=None, n=40):
    """The entry point itself, with one argument off the variant's conditions; returns its status."""
    from pathpyg_amd import _hip
    L = _hip.lib()
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    ptr, idx = i32(n + 1), i32(1)
    dpre, x, w, agg, self_coef = f32(n, m), f32(n, k), f32(m, k), f32(n, k_below), f32(n)
    colsum, dw, dw_below = f32(k), f32(m, k), f32(k, k_below)
    slot = torch.full((n,), -1, dtype=torch.int32, device=DEV) if heavy else None
    sums = f32(1, m) if heavy else None
    ws = torch.empty(int(L.pp_gcn_backward_below_ws_bytes(n)), dtype=torch.uint8, device=DEV)
    p = lambda t_: None if t_ is None else t_.data_ptr()
    rc = L.pp_gcn_backward_below_f32(p(ptr), p(idx), None, n, n if n_self is None else n_self, 0, p(dpre), m, p(self_coef), p(x), k, p(w), fuse_act,
                                     p(slot), p(sums), None, p(colsum), p(dw), p(ws), ws.numel(), drop_p, 1, 2, 0, p(agg), k_below, p(dw_below),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kw", [dict(m=32), dict(k=32), dict(k_below=32), dict(m=128, k=128, k_below=128), dict(fuse_act=0), dict(heavy=True),
                                dict(drop_p=0.25), dict(n_self=30)], ids=str)
def test_backward_below_rejects_what_it_has_no_variant_for(pp, kw):
    """An error, not a wrong answer: the kernel exists for 64/64/64 widths, with the ELU' of the layer below, on a whole graph without hub
    rows and without dropout."""
    assert _raw_call() == 0
    assert _raw_call(**kw) == -2                                       # PP_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- model level
def _bundle(seed, n, e, n_ho, e_ho, f):
    """As tests/test_gpu_dbgnn.py::_bundle (coalesced random graphs with some self loops, mapping "last")."""
    g = torch.Generator().manual_seed(seed)

    def graph(nn, ee):
        ei = torch.randint(0, nn, (2, ee), generator=g)
        ei[:, : ee // 10] = torch.randint(0, nn, (1, ee // 10), generator=g).repeat(2, 1)
        key = torch.unique(ei[0] * nn + ei[1])
        ei = torch.stack((key // nn, key % nn))
        return ei, torch.randint(1, 6, (ei.size(1),), generator=g).float()

    ei, w = graph(n, e)
    ei_h, w_h = graph(n_ho, e_ho)
    ns = torch.randint(0, n, (n_ho, 2), generator=g)
    from oracle import model as om
    data = {
        "num_nodes": n, "num_ho_nodes": n_ho,
        "x": torch.randn(n, f[0], generator=g), "x_h": torch.randn(n_ho, f[1], generator=g),
        "edge_index": ei, "edge_weights": w, "edge_index_higher_order": ei_h, "edge_weights_higher_order": w_h,
        "bipartite_edge_index": om.bipartite_edge_index(ns, "last"),
    }
    return data, torch.randint(0, 3, (n,), generator=g)


N_FO, N_HO = 300, 1500           # first-order graph: 4000 edges (> 8 per row: stays on two kernels); order-2 graph: 6000 edges (<= 8 per row)


@functools.lru_cache(maxsize=None)
def _model_case(n_layers):
    from oracle import dbgnn as od
    hidden = [64] * (n_layers + 1)
    data, y = _bundle(11, N_FO, 4000, N_HO, 6000, (64, 64))
    params = od.init_params(3, (64, 64), hidden, seed=11)
    return data, y, params, hidden, od.loss_and_grads(params, data, y)


def _train_step(pp, n_layers, fuse, monkeypatch, p_dropout=0.0):
    """(logits, loss, {name: grad}, calls of gcn_backward_below, rows of every weight_grad call) of one step through ShardedDBGNN at world 1."""
    from pathpyg_amd import _hip, distributed as pd
    from pathpyg_amd.nn import sharded
    data, y, params, hidden, _ = _model_case(n_layers)
    net = pp.nn.DBGNN(num_classes=3, num_features=(64, 64), hidden_dims=hidden, p_dropout=p_dropout)
    net.load_state_dict(params)
    net = net.to(DEV)
    net.train(p_dropout > 0)
    gdata = pp.Data(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in data.items()}, y=y.to(DEV))
    below_calls, wg_rows = [], []
    real_below, real_wg = _hip.gcn_backward_below, _hip.weight_grad

    def below(*a, **kw):
        below_calls.append(a[3])
        return real_below(*a, **kw)

    def weight_grad(dy, x, want_bias):
        wg_rows.append(dy.size(0))
        return real_wg(dy, x, want_bias)

    with monkeypatch.context() as patch:                               # (undone on exit: a second step counts its own calls only)
        patch.setattr(_hip, "gcn_backward_below", below)
        patch.setattr(_hip, "weight_grad", weight_grad)
        patch.setattr(sharded, "FUSE_FIRST_DW", fuse)
        model = pd.ShardedDBGNN(net)
        shard = model.prepare(gdata)
        out = model(shard).detach().clone()
        assert shard.ho.plan.bwd_idx.numel() <= 8 * N_HO and shard.fo.plan.bwd_idx.numel() > 8 * N_FO
        loss = model.loss(shard)
        loss.backward()
    return out, loss.detach().clone(), {name: p.grad.clone() for name, p in net.named_parameters()}, below_calls, wg_rows


@pytest.mark.parametrize("n_layers", [2, 3])
def test_sharded_dbgnn_fuses_the_first_weight_gradient_and_keeps_its_results(pp, monkeypatch, n_layers):
    """Flag on against flag off and against the oracle; a three-layer stack fuses at index 1 only (its layer 2 keeps the plain kernel)."""
    want_out, want_loss, want_grads = _model_case(n_layers)[4]
    out_off, loss_off, grads_off, below_off, wg_off = _train_step(pp, n_layers, False, monkeypatch)
    out_on, loss_on, grads_on, below_on, wg_on = _train_step(pp, n_layers, True, monkeypatch)
    # the forward pass is untouched
    assert torch.equal(out_on, out_off) and torch.equal(loss_on, loss_off)
    torch.testing.assert_close(out_on.cpu(), want_out, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(loss_on.cpu(), want_loss, rtol=RTOL, atol=ATOL)
    # one fused call for the order-2 stack in place of its first layer's weight_grad; the denser first-order stack keeps its two kernels
    assert below_off == [] and below_on == [N_HO]
    assert wg_on.count(N_HO) == wg_off.count(N_HO) - 1 and wg_on.count(N_FO) == wg_off.count(N_FO) >= 1
    for name in want_grads:
        print(f"[gradient] {name}: on vs oracle needs rtol {gradient_rtol_needed(grads_on[name], want_grads[name]):.2e}, "
              f"on vs off {gradient_rtol_needed(grads_on[name], grads_off[name]):.2e}")
    for name in want_grads:
        assert_gradients_close(grads_on[name], want_grads[name], f"flag on vs the oracle, {name}")
        assert_gradients_close(grads_off[name], want_grads[name], f"flag off vs the oracle, {name}")
        assert_gradients_close(grads_on[name], grads_off[name], f"flag on vs flag off, {name}")


def test_sharded_dbgnn_with_dropout_keeps_the_two_kernel_path(pp, monkeypatch):
    _, _, _, below_calls, wg_rows = _train_step(pp, 2, True, monkeypatch, p_dropout=0.3)
    assert below_calls == [] and wg_rows.count(N_HO) >= 1
