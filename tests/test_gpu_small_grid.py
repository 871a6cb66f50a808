"""The persistent-grid kernels with many tiles per workgroup: ``_hip.launch_share(1)`` shrinks every grid that is sized through
``shared_grid`` to 8 workgroups, so a few thousand rows walk each workgroup's tile loop up to nine times and more — the row-pointer
prefetch one tile ahead, the two LDS tile buffers of k_wide_ws, the chunk prefetch of k_dense_lds that wraps into the next row group,
the per-workgroup dW / column-sum accumulators and the global rows of the dropout epilogues.

Rows per workgroup and loop step (R; tests/small_grid_cases.py states it per shape): 64 for k_gcn_forward 16/32/64, k_gcn_backward (all
variants), the head kernels, k_wide_layer and k_wide_ws; 128 for the 128-wide k_gcn_forward (8 waves); 256 / 128 / 128 for k_dense_lds at
Q = 64 / 128 / 256.  Row counts per kernel: 8 R, 8 R + 1, 24 R - 15, 27 R + 17 and 72 R + R / 2 (``row_counts``).  Every launch under share 1
asserts ``last_persistent_grid() == 8``.

Bars.  Every linear output is computed on inputs for which fp32 arithmetic is exact in any order (tests/small_grid_cases.py proves it per
case from the float64 reference, tests/test_host_logic.py runs that proof without a GPU) and must EQUAL the float64 result, under share 1
and under share 1000.  ``act = 1`` layer outputs and the head's forward pass (expm1) are held to tests/tolerance.py at its default 1e-5,
and their share-1 result must equal their share-1000 result bit for bit: a row is computed by one lane group in a fixed order whichever
workgroup owns it.  The wrappers are called from the test thread: the share is thread-local and autograd would run backward on another.
"""
import pytest
import torch

from tests import small_grid_cases as sg
from tests.tolerance import assert_embeddings_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from pathpyg_amd import _hip
    return _hip


def _dev(t):
    if t is None:
        return None
    return t.to(DEV, torch.float32) if t.is_floating_point() else t.to(DEV)


def _at_both_shares(hip, call, n, r):
    """``call()`` on ``n`` rows (``r`` per workgroup and loop step) at a grid of 8 workgroups and at the default share: ``(small, full)``,
    each a tuple of tensors (None kept).  The full grid has a workgroup per step (more than 8 beyond 8 r rows): the recorded grid is
    this launch's, not an earlier one's."""
    as_tuple = lambda out: out if isinstance(out, tuple) else (out,)
    with hip.launch_share(1):
        small = as_tuple(call())
        assert hip.last_persistent_grid() == 8
    full = as_tuple(call())
    assert (hip.last_persistent_grid() > 8) == (n > 8 * r) and hip.last_persistent_grid() >= 8
    return small, full


def _assert_exact(got, want, what):
    got, want = got.cpu(), want.float()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if not torch.equal(got, want):
        bad = (got != want).reshape(got.size(0), -1).any(1).nonzero().flatten()
        raise AssertionError(f"{what}: {int((got != want).sum())} entries in {bad.numel()} rows differ from the float64 result "
                             f"(rows {bad[:8].tolist()} .. {bad[-1:].tolist()}), max abs diff {float((got - want).abs().max()):.3e}")


def _csr(hip, gr, n, use_val=True, heavy=False):
    ptr, idx, val = _dev(gr.ptr), _dev(gr.idx), _dev(gr.val) if use_val else None
    rows = None
    if heavy:
        rows = hip.HeavyRows(ptr, n, threshold=300)
        assert rows.n_heavy == 2                                      # both long rows go through pp_spmm_heavy_f32, inside tiles of ordinary rows
    return ptr, idx, val, rows


def _cases(shapes):
    return [pytest.param(shape, n, id=f"{'x'.join(map(str, shape))}-n{n}") for shape, r in shapes.items() for n in sg.row_counts(r)]


def test_launch_share_round_trip(hip):
    """pp_set_launch_share returns the previous value; the context manager restores it, also when its body raises."""
    L = hip.lib()
    assert L.pp_set_launch_share(1000) == 1000
    with hip.launch_share(1):
        assert L.pp_set_launch_share(1) == 1
        with hip.launch_share(250):
            assert L.pp_set_launch_share(250) == 250
        assert L.pp_set_launch_share(1) == 1
    assert L.pp_set_launch_share(1000) == 1000
    with pytest.raises(RuntimeError):
        with hip.launch_share(1):
            raise RuntimeError("body")
    assert L.pp_set_launch_share(1000) == 1000
    assert L.pp_set_launch_share(0) == 1000 and L.pp_set_launch_share(5000) == 1          # clamped to 1 .. 1000
    assert L.pp_set_launch_share(1000) == 1000


@pytest.mark.parametrize("shape,n", _cases(sg.FORWARD_SHAPES))
def test_gcn_forward(hip, shape, n):
    """k_gcn_forward (16/32/64 and 128-wide), k_wide_layer, k_wide_ws (kEpi 0): plain with the kept aggregate; without self term and
    values; hub rows; dropout in the epilogue at a global row offset — each without and with the ELU."""
    p, q = shape
    for variant in sg.FORWARD_VARIANTS:
        if variant == "drop" and not hip.gcn_drop_supported(p, q):
            continue
        c = sg.forward_case(p, q, n, variant)
        ptr, idx, val, heavy = _csr(hip, c.graph, n, c.use_val, c.heavy)
        x, sc, w, b = _dev(c.x), _dev(c.self_coef), _dev(c.w), _dev(c.bias)
        want = c.exact["forward"]
        for act in (False, True):
            small, full = _at_both_shares(hip, lambda: hip.gcn_forward(ptr, idx, val, n, x, sc, w, b, act, want_agg=c.want_agg, heavy=heavy, drop=c.drop),
                                          n, sg.FORWARD_SHAPES[shape])
            for share, got in (("share 1", small), ("share 1000", full)):
                what = f"{variant} act={int(act)} {share}"
                if c.want_agg:
                    _assert_exact(got[1], want["agg"][0], f"{what}: agg")
                if act:
                    assert_embeddings_close(got[0], c.y_elu, what=f"{what}: y")
                else:
                    _assert_exact(got[0], want["y"][0], f"{what}: y")
            assert torch.equal(small[0], full[0]), f"{variant} act={int(act)}: a grid of 8 and the full grid give different bits"


def _run_gradient_variants(hip, m, k, n, r, degree, variants, call, names):
    for variant in variants:
        c = sg.backward_case(m, k, n, degree, variant)
        ptr, idx, val, heavy = _csr(hip, c.graph, n, True, c.heavy)
        t = dict(ptr=ptr, idx=idx, val=val, heavy=heavy, dpre=_dev(c.dpre), sc=_dev(c.self_coef), x=_dev(c.x), w=_dev(c.w),
                 n_self=c.n_self if c.n_self != n else None)
        small, full = _at_both_shares(hip, lambda: call(c, t), n, r)
        for share, got in (("share 1", small), ("share 1000", full)):
            for name, tensor in zip(names, got):
                _assert_exact(tensor, c.exact["backward"][name][0], f"{variant} {share}: {name}")


@pytest.mark.parametrize("degree", [4, 12], ids=["capped", "two-wave"])
@pytest.mark.parametrize("shape,n", _cases(sg.BACKWARD_SHAPES))
def test_gcn_backward(hip, shape, n, degree):
    """k_gcn_backward on short rows (nnz <= 8 n: the register-capped kernel at 64 x 64) and long ones: with and without the ELU', on a shard
    (n_self < n_rows), with hub rows, with the dropout of the activation below."""
    m, k = shape
    call = lambda c, t: hip.gcn_backward(t["ptr"], t["idx"], t["val"], n, t["dpre"], t["sc"], t["x"], t["w"], c.fuse, True, heavy=t["heavy"],
                                         n_self=t["n_self"], drop=c.drop)
    _run_gradient_variants(hip, m, k, n, sg.BACKWARD_SHAPES[shape], degree, sg.BACKWARD_VARIANTS, call, ("d_in", "colsum", "dw"))


@pytest.mark.parametrize("shape,n", _cases(sg.INPUT_GRAD_SHAPES))
def test_gcn_input_grad(hip, shape, n):
    """The gradient epilogue (kEpi 1) of the 128-wide k_gcn_forward, k_wide_layer and k_wide_ws: x_act given and None, on a shard, with hub
    rows, with dropout (128-wide shapes); without the column sums the same d_in."""
    m, k = shape
    variants = [v for v in sg.INPUT_GRAD_VARIANTS if v != "drop" or hip.gcn_drop_supported(m, k)]
    call = lambda c, t, colsum=True: hip.gcn_input_grad(t["ptr"], t["idx"], t["val"], n, t["dpre"], t["sc"], t["w"], t["x"] if c.fuse else None, colsum,
                                                        heavy=t["heavy"], n_self=t["n_self"], drop=c.drop)
    _run_gradient_variants(hip, m, k, n, sg.INPUT_GRAD_SHAPES[shape], 4, variants, call, ("d_in", "colsum"))
    _run_gradient_variants(hip, m, k, n, sg.INPUT_GRAD_SHAPES[shape], 4, ["fuse"], lambda c, t: call(c, t, False)[0], ("d_in",))


@pytest.mark.parametrize("n", sg.row_counts(64))
def test_gcn_backward_below(hip, n):
    """The kBelow variant: two sets of per-workgroup weight-gradient accumulators across all tiles of a workgroup."""
    c = sg.backward_case(64, 64, n, 4, "fuse", True)
    ptr, idx, val, _ = _csr(hip, c.graph, n)
    dpre, sc, x, w, below = _dev(c.dpre), _dev(c.self_coef), _dev(c.x), _dev(c.w), _dev(c.agg_below)
    small, full = _at_both_shares(hip, lambda: hip.gcn_backward_below(ptr, idx, val, n, dpre, sc, x, w, below), n, 64)
    for share, got in (("share 1", small), ("share 1000", full)):
        for name, tensor in zip(("colsum", "dw", "dw_below"), got):
            _assert_exact(tensor, c.exact["backward"][name][0], f"{share}: {name}")


@pytest.mark.parametrize("c_out", sg.HEAD_CLASSES)
@pytest.mark.parametrize("widths", sg.HEAD_WIDTHS, ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("n", sg.row_counts(sg.HEAD_ROWS))
def test_head(hip, n, widths, c_out):
    """k_head_forward (1e-5, and the same bits at both grids) and k_head_backward on a stored z (exact)."""
    c = sg.head_case(*widths, c_out, n)
    f = {name: _dev(t) for name, t in c.forward.items()}
    x, deg, w1, w2, wlin, blin = _dev(c.x), _dev(c.deg), _dev(c.w1), _dev(c.w2), _dev(c.wlin), _dev(c.blin)
    small, full = _at_both_shares(hip, lambda: hip.head_forward(f["agg"], x, deg, w1, f["b1"], f["w2"], f["b2"], wlin, blin), n, sg.HEAD_ROWS)
    assert bool((c.z > 0).any()) and bool(((c.z < 0) & (c.z > -0.99)).any())
    for share, got in (("share 1", small), ("share 1000", full)):
        assert_embeddings_close(got[0], c.z, what=f"{share}: z")
        assert_embeddings_close(got[1], c.logits, what=f"{share}: logits")
    assert torch.equal(small[0], full[0]) and torch.equal(small[1], full[1]), "a grid of 8 and the full grid give different bits"
    dlogits, z_in, agg = _dev(c.dlogits), _dev(c.z_in), _dev(c.agg)
    small, full = _at_both_shares(hip, lambda: hip.head_backward(dlogits, z_in, agg, x, deg, w1, w2, wlin, True), n, sg.HEAD_ROWS)
    names = ("d_agg", "dpre_fo", "colsum_fo", "dW1", "dW2", "db1", "db2", "dWlin", "dblin")
    for share, got in (("share 1", small), ("share 1000", full)):
        for name, tensor in zip(names, got):
            _assert_exact(tensor, c.exact["backward"][name][0], f"{share}: {name}")


@pytest.mark.parametrize("transposed", [False, True], ids=["kq", "transposed"])
@pytest.mark.parametrize("shape,n", _cases(sg.DENSE_SHAPES))
def test_dense_lds(hip, shape, n, transposed):
    """k_dense_lds (dense_supported == 3) in both weight orientations: the forward layout with a bias, the gradient layout with ELU' and
    column sums."""
    p, q = shape
    assert hip.dense_supported(p, q) == 3
    c = sg.dense_case(p, q, n)
    weight = _dev(c.w.t().contiguous() if transposed else c.w)
    a, bias, d, y = _dev(c.a), _dev(c.bias), _dev(c.d), _dev(c.y)
    small, full = _at_both_shares(hip, lambda: hip.dense(a, weight, transposed, bias)[0], n, sg.DENSE_SHAPES[shape])
    for share, got in (("share 1", small), ("share 1000", full)):
        _assert_exact(got[0], c.exact["forward"]["out"][0], f"{share}: out")
    small, full = _at_both_shares(hip, lambda: hip.dense(d, weight, transposed, None, grad_act=y, want_colsum=True), n, sg.DENSE_SHAPES[shape])
    for share, got in (("share 1", small), ("share 1000", full)):
        _assert_exact(got[0], c.exact["gradient"]["grad"][0], f"{share}: grad")
        _assert_exact(got[1], c.exact["gradient"]["colsum"][0], f"{share}: colsum")
