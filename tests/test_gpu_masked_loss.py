"""The masked, class-weighted cross-entropy (pp_cross_entropy_masked_f32) and the masked confusion matrix (pp_confusion_f32) on the GPU.

References: ``F.cross_entropy(z[mask], y[mask], weight=w, ignore_index=.., reduction=..)`` on float64 logits on the CPU, with its autograd
gradient, for the loss; a numpy loop over ``np.argmax`` for the confusion matrix.

Rows: n = 8 * 256 * 2 + 37 = 4133 — at the smallest grid (``_hip.launch_share(1)``: 8 workgroups of 256 lanes, one row per lane) every lane
walks its loop twice and 37 lanes a third time; at the default share the grid is 17 workgroups, the last one partial.

Bars (those of tests/test_gpu_value_domain.py's cross-entropy with 1 / n replaced by what multiplies a row here): the loss within 1e-5 of
the reference, relative, without a floor; every gradient entry within ``1e-5 |want| + 2^-22 max(w) / den`` (mean; den = the sum of the
selected rows' weights) or ``1e-5 |want| + 2^-22 max(w)`` (sum); unselected rows and -inf columns exactly 0.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import value_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 8 * 256 * 2 + 37
SELECTIONS = ("random30", "all", "one", "tail", "ignore60", "mask_and_ignore")


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import pathpyg_amd
    return pathpyg_amd


@pytest.fixture(scope="module")
def hip(pp):
    from pathpyg_amd import _hip
    return _hip


def _selection(name, y, g):
    """(target with the unselected rows overwritten, mask or None, ignore_index or None, bool [n] of the selected rows)."""
    n = y.numel()
    rows = torch.arange(n)
    mask, ignore = None, None
    y = y.clone()
    if name == "random30":
        mask = torch.rand(n, generator=g) < 0.3
    elif name == "all":
        mask = torch.ones(n, dtype=torch.bool)
    elif name == "one":
        mask = rows == 1234
    elif name == "tail":
        mask = rows >= n - 20
    elif name == "ignore60":
        ignore = -1
        y[torch.rand(n, generator=g) < 0.6] = -1
    else:
        mask, ignore = torch.rand(n, generator=g) < 0.5, -1
        y[torch.rand(n, generator=g) < 0.3] = -1
    chosen = torch.ones(n, dtype=torch.bool) if mask is None else mask.clone()
    if mask is not None:                                   # rows the mask leaves out: targets no class could have
        out = (~mask).nonzero().flatten()
        y[out[0::2]] = -1
        y[out[1::2]] = 10 ** 9
    if ignore is not None:
        chosen &= y != ignore
    return y, mask, ignore, chosen


def _reference(z, y, mask, weight, ignore, reduction):
    leaf = z.double().requires_grad_(True)
    zz, yy = (leaf, y) if mask is None else (leaf[mask], y[mask])
    loss = F.cross_entropy(zz, yy, weight=None if weight is None else weight.double(), ignore_index=-100 if ignore is None else ignore,
                           reduction=reduction)
    loss.backward()
    return loss.detach(), leaf.grad


def _native(pp, z, y, mask, weight, ignore, reduction):
    leaf = z.to(DEV).requires_grad_(True)
    loss = pp.nn.cross_entropy(leaf, y.to(DEV), mask=None if mask is None else mask.to(DEV), weight=None if weight is None else weight.to(DEV),
                               ignore_index=ignore, reduction=reduction)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_MaskedCrossEntropy")
    loss.backward()
    return loss.detach().cpu().double(), leaf.grad.cpu().double()


def _check(what, z, y, chosen, weight, reduction, got, grad, want, want_grad):
    """The bars of the module docstring; prints each figure before it asserts."""
    w_rows = torch.ones(int(chosen.sum()), dtype=torch.float64) if weight is None else weight.double()[y[chosen]]
    den, max_w = float(w_rows.sum()), 1.0 if weight is None else float(weight.max())
    floor = 2.0 ** -22 * max_w / (den if reduction == "mean" else 1.0)
    err = (grad - want_grad).abs()
    excess = float((err - 1e-5 * want_grad.abs()).max())
    print(f"{what}: loss {float(got)!r}, float64 {float(want)!r}, relative error {float((got - want).abs() / want.abs()):.2e}; "
          f"gradient error beyond 1e-5 |want|: {excess:.2e} (floor {floor:.2e})")
    assert float((got - want).abs()) <= 1e-5 * float(want.abs()), f"{what}: loss {float(got)!r} against {float(want)!r}"
    assert bool((err <= 1e-5 * want_grad.abs() + floor).all()), f"{what}: gradient off by up to {float(err.max()):.3e} (floor {floor:.3e})"
    assert bool((grad[~chosen] == 0).all()), f"{what}: the gradient of an unselected row is not exactly 0"
    hidden = torch.isinf(z)
    hidden[torch.arange(z.size(0))[chosen], y[chosen]] = False
    assert bool((grad[hidden] == 0).all()), f"{what}: dlogits is not exactly 0 in a -inf column"


@pytest.mark.parametrize("c", vc.CE_CLASSES)
@pytest.mark.parametrize("kind", ("spread200", "margin20", "masked"))
def test_masked_loss_matches_float64_torch(pp, kind, c):
    """Every selection x {no weights, 0.5 + rand(C)} x {mean, sum} for one (kind of logits, class count)."""
    z, y0 = vc.cross_entropy_case(kind, N, c)
    g = torch.Generator().manual_seed(7 * c + len(kind))
    weights = (None, 0.5 + torch.rand(c, generator=g))
    for name in SELECTIONS:
        y, mask, ignore, chosen = _selection(name, y0, g)
        if name in ("random30", "ignore60", "mask_and_ignore"):
            assert int(chosen.sum()) > 1000 and bool((torch.bincount(y[chosen], minlength=c) > 0).all())
        for weight in weights:
            for reduction in ("mean", "sum"):
                want, want_grad = _reference(z, y, mask, weight, ignore, reduction)
                got, grad = _native(pp, z, y, mask, weight, ignore, reduction)
                _check(f"{kind} C={c} {name} weight={'yes' if weight is not None else 'no'} {reduction}", z, y, chosen, weight, reduction,
                       got, grad, want, want_grad)


@pytest.mark.parametrize("c", vc.CE_CLASSES)
def test_selected_target_on_a_masked_class_gives_inf(pp, c):
    """``masked_target``: every 97th row has -inf at its target.  With such rows selected the loss is +inf (as torch's); with them left
    out it is finite and within the bar."""
    z, y0 = vc.cross_entropy_case("masked_target", N, c)
    g = torch.Generator().manual_seed(c)
    poisoned = torch.zeros(N, dtype=torch.bool)
    poisoned[::97] = True
    some = torch.rand(N, generator=g) < 0.3
    for mask, finite in ((some | poisoned, False), (some & ~poisoned, True)):
        y = y0.clone()
        y[~mask] = -1
        want, want_grad = _reference(z, y, mask, None, None, "mean")
        got, grad = _native(pp, z, y, mask, None, None, "mean")
        print(f"masked_target C={c} finite={finite}: loss {float(got)!r}, float64 {float(want)!r}")
        if finite:
            assert math.isfinite(float(want))
            _check(f"masked_target C={c} without the poisoned rows", z, y, mask, None, "mean", got, grad, want, want_grad)
        else:
            assert float(want) == math.inf and float(got) == math.inf


def test_empty_selection_gives_nan_loss_and_zero_gradient(pp):
    z, y = vc.cross_entropy_case("spread200", N, 8)
    for kwargs in (dict(mask=torch.zeros(N, dtype=torch.bool, device=DEV)), dict(ignore_index=-1)):
        target = y.to(DEV) if "mask" in kwargs else torch.full((N,), -1, dtype=torch.int64, device=DEV)
        leaf = z.to(DEV).requires_grad_(True)
        loss = pp.nn.cross_entropy(leaf, target, **kwargs)
        loss.backward()
        assert math.isnan(float(loss.detach())) and bool((leaf.grad == 0).all())


def test_out_of_range_target_raises_only_when_selected(pp):
    z, y = vc.cross_entropy_case("margin20", N, 13)
    mask = torch.rand(N, generator=torch.Generator().manual_seed(0)) < 0.3
    inside, outside = int(mask.nonzero()[5]), int((~mask).nonzero()[5])
    for value in (10 ** 9, 13, -1):
        bad = y.clone()
        bad[inside] = value
        with pytest.raises(IndexError):
            pp.nn.cross_entropy(z.to(DEV), bad.to(DEV), mask=mask.to(DEV))
        fine = y.clone()
        fine[outside] = value
        assert math.isfinite(float(pp.nn.cross_entropy(z.to(DEV), fine.to(DEV), mask=mask.to(DEV))))
    # the kernel itself counts such a row, gives it a zero gradient row and leaves it out of the sums
    bad = y.clone()
    bad[inside] = 10 ** 9
    sums, raw = pp._hip.cross_entropy_masked(z.to(DEV), bad.to(DEV), mask.to(DEV))
    assert sums.counts.tolist() == [int(mask.sum()), 1] and bool((raw[inside] == 0).all())
    assert float(sums.values[1]) == float(mask.sum()) - 1


def test_same_bits_on_every_call_and_gradient_independent_of_the_grid(hip):
    z, y = vc.cross_entropy_case("spread200", N, 8)
    g = torch.Generator().manual_seed(3)
    mask, weight = (torch.rand(N, generator=g) < 0.3).to(DEV), (0.5 + torch.rand(8, generator=g)).to(DEV)
    z, y = z.to(DEV), y.to(DEV)
    first, raw_first = hip.cross_entropy_masked(z, y, mask, weight)
    again, raw_again = hip.cross_entropy_masked(z, y, mask, weight)
    assert hip.last_persistent_grid() == 17
    assert torch.equal(first.values.view(torch.int32), again.values.view(torch.int32)) and torch.equal(first.counts, again.counts)
    assert torch.equal(raw_first.view(torch.int32), raw_again.view(torch.int32))
    with hip.launch_share(1):
        small, raw_small = hip.cross_entropy_masked(z, y, mask, weight)
        assert hip.last_persistent_grid() == 8
    with hip.launch_share(1000):
        full, raw_full = hip.cross_entropy_masked(z, y, mask, weight)
        assert hip.last_persistent_grid() == 17
    assert torch.equal(raw_small.view(torch.int32), raw_full.view(torch.int32))
    assert torch.equal(small.counts, full.counts)
    a, b = float(small.values[2]), float(full.values[2])
    print(f"mean loss at a grid of 8: {a!r}, at 17: {b!r}")
    assert abs(a - b) <= 1e-5 * abs(b)


@pytest.mark.parametrize("c", vc.CE_CLASSES)
def test_all_true_mask_agrees_with_the_unmasked_kernel(pp, hip, c):
    z, y = vc.cross_entropy_case("margin20", N, c)
    z, y = z.to(DEV), y.to(DEV)
    want, want_grad = hip.cross_entropy(z, y)
    leaf = z.clone().requires_grad_(True)
    got = pp.nn.cross_entropy(leaf, y, mask=torch.ones(N, dtype=torch.bool, device=DEV))
    got.backward()
    want, want_grad, got, grad = want.cpu().double(), want_grad.cpu().double(), got.detach().cpu().double(), leaf.grad.cpu().double()
    err = (grad - want_grad).abs()
    print(f"C={c}: masked {float(got)!r}, unmasked {float(want)!r}; largest gradient difference {float(err.max()):.2e}")
    assert float((got - want).abs()) <= 1e-5 * float(want.abs())
    assert bool((err <= 1e-5 * want_grad.abs() + 2.0 ** -22 / N).all())


def _scores(conf):
    conf = conf.astype(np.float64)
    support, predicted, hit = conf.sum(1), conf.sum(0), np.diag(conf)
    recall = [hit[k] / support[k] for k in range(len(hit)) if support[k] > 0]
    f1 = [2 * hit[k] / (support[k] + predicted[k]) for k in range(len(hit)) if support[k] + predicted[k] > 0]
    return support, hit.sum() / support.sum(), float(np.mean(recall)), float(np.mean(f1))


@pytest.mark.parametrize("c", (2, 13, 64))
def test_evaluate_matches_numpy(pp, hip, c):
    """Logits in multiples of 0.5 (ties at the maximum), one selected row with a NaN; confusion matrix at a grid of 8 and at the default
    grid against a numpy loop, the scores against the same formulas in numpy."""
    g = torch.Generator().manual_seed(100 + c)
    z = torch.round(torch.randn(N, c, generator=g) * 2) / 2
    y = torch.randint(0, c, (N,), generator=g)
    z[7, c // 2] = math.nan
    mask = torch.rand(N, generator=g) < 0.5
    mask[7] = True
    for use_mask, ignore in ((True, None), (False, -1), (True, -1)):
        target = y.clone()
        chosen = mask.clone() if use_mask else torch.ones(N, dtype=torch.bool)
        if use_mask:
            target[~mask] = 10 ** 9
        if ignore is not None:
            dropped = torch.rand(N, generator=g) < 0.3
            dropped[7] = False
            target[dropped] = ignore
            chosen &= ~dropped
        zn, yn = z.numpy(), target.numpy()
        ties = 0
        want = np.zeros((c, c), dtype=np.int64)
        for i in np.flatnonzero(chosen.numpy()):
            want[yn[i], np.argmax(zn[i])] += 1
            ties += int((zn[i] == np.nanmax(zn[i])).sum() > 1)
        assert ties > 0 and want[yn[7], c // 2] > 0
        args = (z.to(DEV), target.to(DEV), mask.to(DEV) if use_mask else None, ignore)
        with hip.launch_share(1):
            small = hip.confusion(*args)
            assert hip.last_persistent_grid() == 8
        with hip.launch_share(1000):
            full = hip.confusion(*args)
            assert hip.last_persistent_grid() == 17
        assert np.array_equal(small.cpu().numpy(), want) and np.array_equal(full.cpu().numpy(), want)
        res = pp.nn.evaluate(args[0], args[1], mask=args[2], ignore_index=ignore)
        assert res["confusion"].is_cuda and res["confusion"].dtype == torch.int64 and np.array_equal(res["confusion"].cpu().numpy(), want)
        support, accuracy, balanced, macro_f1 = _scores(want)
        assert np.array_equal(res["support"].numpy(), support.astype(np.int64))
        assert abs(res["accuracy"] - accuracy) <= 1e-12 and abs(res["balanced_accuracy"] - balanced) <= 1e-12
        assert abs(res["macro_f1"] - macro_f1) <= 1e-12
    with pytest.raises(IndexError):
        pp.nn.evaluate(z.to(DEV), torch.full((N,), c, dtype=torch.int64, device=DEV), mask=mask.to(DEV))


# ---------------------------------------------------------------------------------------------------------------- end to end
RTOL, ATOL = 1e-5, 2e-6                                   # the bars of tests/test_gpu_dbgnn.py


def _bundle(seed, n, e, n_ho, e_ho, f):
    """The bundle of tests/test_gpu_dbgnn.py (mapping "last", with loops), restated."""
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


def test_training_step_on_a_node_split_matches_the_oracle_without_gather_or_read_back(pp):
    from oracle import dbgnn as od
    f, hidden = (64, 64), [64, 64, 64]
    data, y = _bundle(1, 200, 3000, 900, 4000, f)
    params = od.init_params(3, f, hidden, seed=1)
    gdata = pp.Data(**{k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in data.items()})
    gdata.y = y.to(DEV)
    pp.utils.random_node_split(gdata, num_val=0.5, generator=torch.Generator().manual_seed(5))
    assert gdata.train_mask.is_cuda and int(gdata.train_mask.sum()) == 100 and int(gdata.val_mask.sum()) == 100
    want_out, want_loss, want_grads = od.loss_and_grads(params, data, y, gdata.train_mask.cpu())

    model = pp.nn.DBGNN(num_classes=3, num_features=f, hidden_dims=hidden, p_dropout=0.0)
    model.load_state_dict(params, strict=True)
    model = model.to(DEV)
    out = model(gdata)
    loss = pp.nn.cross_entropy(out, gdata.y, mask=gdata.train_mask)
    loss.backward()
    torch.testing.assert_close(out.detach().cpu(), want_out, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(loss.detach().cpu(), want_loss, rtol=RTOL, atol=ATOL)
    for name, p in model.named_parameters():
        scale = float(want_grads[name].abs().max()) + 1e-12
        torch.testing.assert_close(p.grad.cpu(), want_grads[name], rtol=RTOL * 10, atol=max(ATOL, 2e-5 * scale), msg=lambda s_: f"{name}: {s_}")
    scores = pp.nn.evaluate(out, gdata.y, mask=gdata.val_mask)
    assert int(scores["support"].sum()) == 100

    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
        loss = pp.nn.cross_entropy(model(gdata), gdata.y, mask=gdata.train_mask)
        loss.backward()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert any("k_cross_entropy_masked" in k for k in names), names
    gather = [k for k in names if "nonzero" in k.lower() or "index_put" in k.lower() or k.startswith("aten::index") or "index_kernel" in k.lower()
              or "indexing" in k.lower()]
    copies = [k for k in names if "dtoh" in k.lower() or "_local_scalar_dense" in k or k == "aten::item"]
    assert not gather and not copies, (gather, copies, names)
