"""What the kernels do to VALUES: the ELU and ELU' epilogues through every entry point at the ends of the fp32 range, the cross-entropy
at large spreads, on confident rows and with masked classes, and Adam's constants over 100 steps of one-signed gradients.

ELU / ELU'.  tests/value_cases.py builds, per kernel family, inputs for which everything in front of the epilogue is exact in fp32 (one
unit term per sum; tests/test_host_logic.py proves it without a GPU), so the output isolates the epilogue, and lays the value grids out so
that every value stands in every column.  Forward outputs are held to float64 ``expm1`` element by element, PURELY relatively (no rms floor):
zeros exact, positive inputs bit for bit, negative ones within the project's 1e-5 and within 4 x the bound documented in csrc/pp_common.h
(3e-7 + 5e-8).  ELU' outputs are held to float64 ``g * (y > 0 ? 1 : y + 1)`` within 2^-23 relative (exactly 0 where y = -1), column sums
within n * 2^-24 * sum |terms|.  The entry points without dropout that are not called here by name (pp_gcn_forward_f32,
pp_gcn_input_grad_f32, pp_spmm_act_backward_f32) forward to their ``_drop`` forms with p = 0, which the wrappers call; pp_gcn_backward_f32
(row lengths unknown: the two-wave kernel) is called directly.

Measured on an MI355X, largest relative error of the ELU over all forward entry points: polynomial branch 9.3e-8, exponential branch
1.2e-7 (``_check_elu`` prints them per entry point); the documented bound is 3.5e-7.  No ELU or ELU' epilogue missed its bar.

Cross-entropy (reference: ``F.cross_entropy`` on float64 logits, CPU, with its autograd gradient; the loss at rtol 1e-5 without a floor,
the gradient within 1e-5 |want| + 2^-22 / n).  Measured relative error of the loss on the confident rows (n = 1000, C in {2, 8, 13, 64}):
at most 1.3e-7 with the target raised by 12, at most 1.5e-7 with 20; at most 9.4e-8 at randn * 40 and * 200.  The kernel used to return
-log(softmax[y]): 4.9e-2 .. 1.3e-1 off at randn * 40, 0.63 .. 0.79 at randn * 200, 7.2e-6 .. 1.3e-4 at a margin of 12, 0.42 .. 0.69 at 20,
and a finite loss (2.3 .. 8.3) where torch gives inf for a target on a masked class.  Its gradient at the target class, softmax[y] - 1,
missed the gradient bar on the confident rows (3.4e-7 / n: the sum of C terms above 1 rounds to 2^-23 each time) and is now
-(sum of the other classes) / sum.

Adam (100 steps, lr 1e-2, weight decay 5e-4, gradients 0.5 + 0.1 randn): largest deviation from the float64 recurrence 2.279e-6 for
``pp.nn.optim.Adam`` and 2.279e-6 for ``torch.optim.Adam`` on the same fp32 inputs (ratio 1.00); with 1.f - b1 and 1.f - b2 formed from
the rounded betas the first was 8.081e-6 (ratio 3.55).
"""
import pytest
import torch

from tests import value_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DOCUMENTED = 3e-7 + 5e-8                               # csrc/pp_common.h, elu_fast: 1 ulp of the exponential over 0.22, plus the truncation
WORST = {"polynomial": 0.0, "exponential": 0.0}


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from pathpyg_amd import _hip
    return _hip


def _dev(t):
    return None if t is None else t.to(DEV)


def _check_elu(got, pre, what, factor=None):
    """``got`` against ELU(``pre``) (times the dropout factors in {0, 2}): zeros exact, positive inputs bit for bit, negative ones within
    1e-5 and within 4 x DOCUMENTED, element by element and purely relative."""
    got = got.cpu()
    assert got.shape == pre.shape and got.dtype == torch.float32, what
    want = vc.elu_reference(pre)
    kept = torch.ones_like(pre, dtype=torch.bool)
    if factor is not None:
        want, kept = want * factor.double(), factor != 0
        assert bool((got[~kept] == 0).all()), f"{what}: a dropped entry is not 0"
    positive, zero, negative = (pre > 0) & kept, (pre == 0) & kept, (pre < 0) & kept
    assert torch.equal(got[positive].double(), want[positive]), f"{what}: a positive input does not come back bit for bit"
    assert bool((got[zero] == 0).all()), f"{what}: ELU(0) is not 0"
    rel = (got.double() - want).abs() / want.abs()
    worst = {}
    for branch, where in (("polynomial", negative & (pre > -0.25)), ("exponential", negative & (pre <= -0.25))):
        assert bool(where.any()), f"{what}: no input on the {branch} branch"
        at = int(torch.where(where, rel, torch.zeros_like(rel)).argmax())
        worst[branch] = (float(rel.flatten()[at]), float(pre.flatten()[at]))
        WORST[branch] = max(WORST[branch], worst[branch][0])
    print(f"ELU {what}: largest relative error " + ", ".join(f"{b} {e:.2e} at x = {x:.6g}" for b, (e, x) in worst.items()))
    for branch, (err, x) in worst.items():
        assert err <= 1e-5, f"{what}: {branch} branch {err:.2e} relative at x = {x!r}"
        assert err <= 4 * DOCUMENTED, f"{what}: {branch} branch {err:.2e} relative at x = {x!r}: 4 x the bound csrc/pp_common.h documents is {4 * DOCUMENTED:.1e}"


def _check_elu_grad(got, front, act, what, factor=None, colsum=None, scale=None):
    """``got`` against ``front * ELU'(act)`` in float64 (times the dropout factors, times a per-row power of two ``scale``): 2^-23 relative per
    element, exactly 0 where act = -1; ``colsum`` against the float64 column sums within n * 2^-24 * sum |terms|."""
    got = got.cpu()
    want = front.double() * vc.elu_grad_reference(act)
    if factor is not None:
        want = want * factor.double()
    if scale is not None:
        want = want * scale.double().unsqueeze(1)
    assert got.shape == want.shape and got.dtype == torch.float32, what
    assert bool((act == -1).any()) and bool((got[act == -1] == 0).all()), f"{what}: not exactly 0 where the stored activation is -1"
    err, bound = (got.double() - want).abs(), 2.0 ** -23 * want.abs()
    if not bool((err <= bound).all()):
        at = int((err - bound).argmax())
        raise AssertionError(f"{what}: {int((err > bound).sum())} entries beyond 2^-23 relative; y = {float(act.flatten()[at])!r}: got "
                             f"{float(got.flatten()[at])!r}, want {float(want.flatten()[at])!r}")
    if colsum is not None:
        _check_sums(colsum, want.sum(0), want.abs().sum(0), want.size(0), f"{what}: column sums")
    return want


def _check_sums(got, want, terms, n, what):
    err = (got.cpu().double() - want).abs()
    bound = n * 2.0 ** -24 * terms
    assert got.shape == want.shape and bool((err <= bound).all()), f"{what}: off by up to {float((err / terms).max()):.2e} of sum |terms| (bound {n * 2.0 ** -24:.2e})"


# ---------------------------------------------------------------------------------------------------------------- ELU, forward
@pytest.mark.parametrize("style", ["neighbour", "self"])
@pytest.mark.parametrize("f", [64, 7], ids=["v4-64", "s1-7"])
def test_spmm_elu(hip, f, style):
    """pp_spmm_f32 with act = 1: k_spmm_v4 (F = 64) and k_spmm_s1 (F = 7)."""
    c = vc.spmm_case(512, f, style)
    y = hip.spmm(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.x), _dev(c.self_coef), None, _dev(c.bias), True)
    _check_elu(y, c.pre, f"spmm F={f} {style}")


@pytest.mark.parametrize("style", ["neighbour", "self"])
@pytest.mark.parametrize("shape", vc.FORWARD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gcn_forward_elu(hip, shape, style):
    """pp_gcn_forward_f32 at 16/32/64 and the 128-wide shapes, pp_wide_layer_f32 epilogue 0 at the shapes with a side of 256."""
    p, q = shape
    assert hip.gcn_fused_supported(p, q) != 0
    c = vc.gcn_forward_case(512, p, q, style)
    y = hip.gcn_forward(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.x), _dev(c.self_coef), _dev(c.w), _dev(c.bias), True)
    _check_elu(y, c.pre, f"gcn_forward {p}x{q} {style}")


@pytest.mark.parametrize("shape", [(64, 64), (128, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gcn_forward_drop_elu(hip, shape):
    """pp_gcn_forward_drop_f32 at p = 1/2: ELU(pre) * 2 where kept, 0 where dropped."""
    p, q = shape
    c = vc.gcn_forward_case(1024, p, q, "neighbour")
    y = hip.gcn_forward(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.x), _dev(c.self_coef), _dev(c.w), _dev(c.bias), True, drop=vc.DROP)
    _check_elu(y, c.pre, f"gcn_forward_drop {p}x{q}", factor=vc.drop_factors(c.n, q))


@pytest.mark.parametrize("which", ["a", "p"])
@pytest.mark.parametrize("f", [64, 20])
def test_bip_combine_elu(hip, f, which):
    c = vc.bip_combine_case(512, f, which)
    y = hip.bip_combine(_dev(c.a), _dev(c.p), _dev(c.deg), _dev(c.bias))
    _check_elu(y, c.pre, f"bip_combine F={f} pre = {which}")


@pytest.mark.parametrize("which", ["agg", "x"])
@pytest.mark.parametrize("widths", vc.HEAD_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_head_forward_elu(hip, widths, which):
    """pp_dbgnn_head_forward_f32: z with pre = agg (deg = 0, W1 a selection) and with pre = x (deg = 1, agg = 0, W2 a selection)."""
    c = vc.head_forward_case(512, *widths, 8, which)
    z, logits = hip.head_forward(_dev(c.agg), _dev(c.x), _dev(c.deg), _dev(c.w1), _dev(c.b1), _dev(c.w2), _dev(c.b2), _dev(c.wlin), _dev(c.blin))
    _check_elu(z, c.pre, f"head_forward {widths} pre = {which}")
    assert bool(torch.isfinite(logits).all())


# ---------------------------------------------------------------------------------------------------------------- ELU', backward
@pytest.mark.parametrize("f", [64, 7])
def test_act_backward(hip, f):
    c = vc.elementwise_case(512, f, 3)
    dpre, dbias = hip.act_backward(_dev(c.g), _dev(c.y), True, True, True)
    _check_elu_grad(dpre, c.pre, c.act, f"act_backward F={f}", colsum=dbias)


def test_bip_combine_backward(hip):
    """dA = dY ELU'(Y), dP = deg dA (deg in {1, 2, 4}), dbias = column sums of dP."""
    c = vc.elementwise_case(512, 64, 3)
    da, dp, db = hip.bip_combine_backward(_dev(c.g), _dev(c.y), _dev(c.deg), True)
    _check_elu_grad(da, c.pre, c.act, "bip_combine_backward dA")
    _check_elu_grad(dp, c.pre, c.act, "bip_combine_backward dP", colsum=db, scale=c.deg)


def test_dropout_act_backward(hip):
    c = vc.elementwise_case(1024, 64, 4, dropped=True)
    p, seed, tag, row0 = vc.DROP
    dpre, dbias = hip.dropout_act_backward(_dev(c.g), _dev(c.y), p, seed, tag, row0, None, True, True)
    _check_elu_grad(dpre, c.pre, c.act, "dropout_act_backward", factor=c.factor, colsum=dbias)


@pytest.mark.parametrize("dropped", [False, True], ids=["plain", "drop"])
def test_spmm_act_backward(hip, dropped):
    """pp_spmm_act_backward_f32 / pp_spmm_act_backward_drop_f32."""
    c = vc.gradient_case(1024 if dropped else 512, 64, 64, 5, "neighbour", dropped)
    dx, colsum = hip.spmm_act_backward(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.d), _dev(c.y), True, drop=vc.DROP if dropped else None)
    _check_elu_grad(dx, c.pre, c.act, f"spmm_act_backward dropped={dropped}", factor=c.factor, colsum=colsum)


@pytest.mark.parametrize("shape,kind", [((64, 64), 1), ((8, 64), 2)], ids=["64x64", "narrow-8x64"])
def test_dense_grad_act(hip, shape, kind):
    """pp_dense_f32 with grad_act on the register-resident kernel and on pp_dense_narrow_f32."""
    m, k = shape
    assert hip.dense_supported(m, k) == kind
    c = vc.gradient_case(512, m, k, m + k, "self")
    out, colsum = hip.dense(_dev(c.d), _dev(c.w), False, None, grad_act=_dev(c.y), want_colsum=True)
    _check_elu_grad(out, c.pre, c.act, f"dense {m}x{k} grad_act", colsum=colsum)


@pytest.mark.parametrize("shape", [(64, 64), (16, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_backward(hip, shape):
    m, k = shape
    c = vc.gradient_case(512, m, k, m + k, "self")
    d_in, colsum, _, _ = hip.dense_backward(_dev(c.d), _dev(c.y), _dev(c.w), True, True, True, False)
    _check_elu_grad(d_in, c.pre, c.act, f"dense_backward {m}x{k}", colsum=colsum)


def _gcn_backward_plain(hip, c):
    """pp_gcn_backward_f32 itself: the number of CSR entries unknown, hence the two-wave kernel at every shape."""
    from pathpyg_amd import _lib
    L, p = _lib.lib(), hip._p
    m, k = c.w.shape
    t = {name: _dev(getattr(c, name)) for name in ("ptr", "idx", "val", "d", "self_coef", "y", "w")}
    with torch.cuda.device(DEV):
        d_in, colsum, dw = torch.empty((c.n, k), device=DEV), torch.empty(k, device=DEV), torch.empty((m, k), device=DEV)
        ws = hip._workspace(L.pp_gcn_backward_ws_bytes(c.n), torch.device(DEV))
        _lib.check(L.pp_gcn_backward_f32(p(t["ptr"]), p(t["idx"]), p(t["val"]), c.n, c.n, p(t["d"]), m, p(t["self_coef"]), p(t["y"]), k, p(t["w"]), 1,
                                         None, None, p(d_in), p(colsum), p(dw), p(ws), ws.numel(), hip._stream()), "pp_gcn_backward_f32")
    return d_in, colsum, dw


@pytest.mark.parametrize("entry", ["plain", "nnz", "drop"])
def test_gcn_backward(hip, entry):
    """pp_gcn_backward_f32 (two-wave kernel), pp_gcn_backward_nnz_f32 on the capped path (nnz = n <= 8 n at 64 x 64) and
    pp_gcn_backward_drop_f32, each with fuse_act."""
    dropped = entry == "drop"
    c = vc.gradient_case(1024 if dropped else 512, 64, 64, 5 if dropped else 128, "neighbour", dropped)
    if entry == "plain":
        d_in, colsum, _ = _gcn_backward_plain(hip, c)
    else:
        assert int(c.idx.numel()) <= 8 * c.n
        d_in, colsum, _ = hip.gcn_backward(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.d), _dev(c.self_coef), _dev(c.y), _dev(c.w), True, True,
                                           drop=vc.DROP if dropped else None)
    _check_elu_grad(d_in, c.pre, c.act, f"gcn_backward {entry}", factor=c.factor, colsum=colsum)


@pytest.mark.parametrize("shape", [(16, 64), (64, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gcn_backward_other_widths(hip, shape):
    m, k = shape
    c = vc.gradient_case(512, m, k, m + k, "neighbour")
    d_in, colsum, _ = hip.gcn_backward(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.d), _dev(c.self_coef), _dev(c.y), _dev(c.w), True, True)
    _check_elu_grad(d_in, c.pre, c.act, f"gcn_backward {m}x{k}", colsum=colsum)


def test_gcn_backward_below(hip):
    """pp_gcn_backward_below_f32 never stores d_in: its column sums, and dW_below = d_in^T agg_below with agg_below[r] the unit vector
    r mod 64 — the sums of d_in over the n / 64 rows of one residue, held to n / 64 * 2^-24 * sum |terms|."""
    c = vc.gradient_case(512, 64, 64, 128, "neighbour")
    below = torch.zeros(c.n, 64)
    below[torch.arange(c.n), torch.arange(c.n) % 64] = 1.0
    colsum, _, dw_below = hip.gcn_backward_below(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.d), _dev(c.self_coef), _dev(c.y), _dev(c.w), _dev(below))
    want = c.pre.double() * vc.elu_grad_reference(c.act)
    _check_sums(colsum, want.sum(0), want.abs().sum(0), c.n, "gcn_backward_below: column sums")
    # (each entry of dW_below has n / 64 non-zero terms: one rounding in each, one per addition)
    _check_sums(dw_below, want.t() @ below.double(), want.abs().t() @ below.double(), c.n // 64, "gcn_backward_below: dW_below")


@pytest.mark.parametrize("shape", [(128, 128), (256, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gcn_input_grad(hip, shape):
    """pp_gcn_input_grad_f32 with fuse_act at 128 x 128 and, at 256 x 256, pp_wide_layer_f32 epilogue 1."""
    m, k = shape
    c = vc.gradient_case(512, m, k, m + k, "neighbour")
    d_in, colsum = hip.gcn_input_grad(_dev(c.ptr), _dev(c.idx), _dev(c.val), c.n, _dev(c.d), _dev(c.self_coef), _dev(c.w), _dev(c.y), True)
    _check_elu_grad(d_in, c.pre, c.act, f"gcn_input_grad {m}x{k}", colsum=colsum)


@pytest.mark.parametrize("which", ["z", "x"])
@pytest.mark.parametrize("widths", vc.HEAD_WIDTHS, ids=lambda w: "x".join(map(str, w)))
def test_head_backward(hip, widths, which):
    """pp_dbgnn_head_backward_f32, both ELU' factors: ELU'(z) through d_agg (every column of z: one offset of the selection W1 per
    Hb / Ha), ELU'(x) through dpre_fo and its column sums."""
    ha, hx, hb = widths
    for offset in range(hb // ha if which == "z" else 1):
        c = vc.head_backward_case(512, ha, hx, hb, 8, which, offset)
        out = hip.head_backward(_dev(c.dlogits), _dev(c.z), _dev(c.agg), _dev(c.x), _dev(c.deg), _dev(c.w1), _dev(c.w2), _dev(c.wlin), True)
        if which == "z":
            _check_elu_grad(out[0], c.pre, c.act, f"head_backward {widths} d_agg, offset {offset}")
        else:
            _check_elu_grad(out[1], c.pre, c.act, f"head_backward {widths} dpre_fo", colsum=out[2])


def test_elu_error_report(hip):
    """The largest relative ELU error per branch over the forward tests of this run (what the module docstring and csrc/pp_common.h record)."""
    print("ELU over all forward entry points of this run: " + ", ".join(f"{b} branch {e:.2e}" for b, e in WORST.items()))
    assert max(WORST.values()) <= 4 * DOCUMENTED


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
def _run_cross_entropy(hip, kind, n, c):
    z, y = vc.cross_entropy_case(kind, n, c)
    want, want_grad = vc.cross_entropy_reference(z, y)
    got, grad = hip.cross_entropy(z.to(DEV), y.to(DEV))
    got, grad = got.cpu().double(), grad.cpu().double()
    print(f"cross-entropy {kind} n={n} C={c}: loss {float(got)!r}, float64 {float(want)!r}, relative error {float((got - want).abs() / want):.2e}")
    if kind == "masked_target":
        assert bool(torch.isinf(want)) and float(got) == float("inf"), f"a target on a masked class: loss {float(got)!r}, torch gives inf"
    else:
        assert float((got - want).abs()) <= 1e-5 * float(want.abs()), f"loss {float(got)!r} against {float(want)!r}"
    err = (grad - want_grad).abs()
    assert bool((err <= 1e-5 * want_grad.abs() + 2.0 ** -22 / n).all()), f"gradient off by up to {float(err.max()) * n:.2e} / n"
    if kind.startswith("masked"):
        masked = torch.isinf(z)
        masked[torch.arange(n), y] = False
        assert bool(masked.any()) and bool((grad[masked] == 0).all()), "dlogits is not exactly 0 in a masked column"


@pytest.mark.parametrize("c", vc.CE_CLASSES)
@pytest.mark.parametrize("kind", vc.CE_KINDS)
def test_cross_entropy_value_domain(hip, kind, c):
    """Logits randn * 40 and * 200; the target class raised by 12 and by 20; -inf in non-target columns; a target on a masked class."""
    _run_cross_entropy(hip, kind, 1000, c)


def test_cross_entropy_value_domain_many_rows(hip):
    _run_cross_entropy(hip, "spread40", 100_003, 8)
    _run_cross_entropy(hip, "margin12", 100_003, 8)


# ---------------------------------------------------------------------------------------------------------------- Adam
def test_adam_constants_do_not_drift(hip):
    """100 steps on one-signed gradients against the float64 recurrence.  The bar is measured: ``pp.nn.optim.Adam`` may deviate at most twice
    as far as ``torch.optim.Adam`` does on the same fp32 inputs — two fp32 evaluations of one recurrence differ by rounding order, not by a
    factor.  Measured: 2.279e-6 against torch's 2.279e-6 (ratio 1.00); with 1.f - b1 and 1.f - b2 formed from the rounded betas it was
    8.081e-6 (ratio 3.55)."""
    import pathpyg_amd as pp
    init, grads = vc.adam_inputs()
    want = vc.adam_reference(init, grads, **vc.ADAM)
    mine = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    theirs = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt, opt_torch = pp.nn.optim.Adam(mine, **vc.ADAM), torch.optim.Adam(theirs, **vc.ADAM)
    for gs in grads:
        for a, b, g in zip(mine, theirs, gs):
            a.grad, b.grad = g.to(DEV), g.to(DEV)
        opt.step()
        opt_torch.step()
    deviation = lambda ps: max(float((p.detach().cpu().double() - w).abs().max()) for p, w in zip(ps, want))
    dev_mine, dev_torch = deviation(mine), deviation(theirs)
    print(f"Adam, {vc.ADAM_STEPS} steps: largest deviation from float64 {dev_mine:.3e} (pp.nn.optim.Adam), {dev_torch:.3e} (torch.optim.Adam), ratio {dev_mine / dev_torch:.2f}")
    assert dev_torch > 0 and dev_mine <= 2 * dev_torch
