"""Inputs and float64 references of tests/test_gpu_small_grid.py: the persistent-grid kernels at a grid of 8 workgroups.

Plain torch-CPU code (no GPU, no library call), so that tests/test_host_logic.py can run the generators and their exactness condition
where no GPU is present.

EXACT INPUTS.  Every linear output (aggregates, ``act = 0`` layer outputs, input gradients, every dW / db / column sum) is evaluated on
inputs for which fp32 arithmetic is exact in ANY order of summation: features are integers in [-2, 2], gradients lie in {-1, 0, 1}, edge
values in {1/2, 1, 3/2}, self coefficients are multiples of 1/4 in [0, 1], weights lie in {-1, -1/2, 0, 1/2, 1}, biases are multiples of 1/4,
stored activations lie in {-1/2, 1} (so ELU' is 1/2 or 1), ``deg`` holds small integers and dropout runs at p = 1/2 (scale 2).  Every term
of an output and therefore every partial sum of any grouping is then a multiple of ``1 / den`` (``den`` a power of two) and no larger in
magnitude than the sum of the terms' magnitudes: if that sum times ``den`` stays below 2^24, every partial sum is an fp32 number and the
fp32 result IS the float64 result.  :func:`exactness` proves both conditions from the float64 evaluation alone (the second one from the
same formulas on the inputs' magnitudes); a generator whose sums over all rows would break the bound thins its gradients (fewer non-zero
entries) until it holds and fails if it never does.
"""
import functools
import types

import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)
DROP = (0.5, 987654321, 65, 2 ** 33 + 5)              # (p, seed, tag, row0): global rows far from 0, beyond 32 bits
LONG_ROW = 600                                       # entries of the two long rows: more than the prefetched pairs, one index chunk and HeavyRows(threshold=300)
WEIGHTS = (-1.0, -0.5, 0.0, 0.5, 1.0)
DENSITIES = (0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625)


def row_counts(r):
    """Rows for a kernel whose workgroup covers ``r`` rows per loop step, at a grid of 8: one step each with nothing behind it; a second
    step of one row for one workgroup; three steps each (odd: double buffers end in their first buffer) with a ragged last tile; four steps
    for some and three for others, one of the fourth a full tile plus a one-row tile; nine or more steps."""
    return [8 * r, 8 * r + 1, 24 * r - 15, 27 * r + 17, 72 * r + r // 2]


# ---------------------------------------------------------------------------------------------------------------- exactness
def exactness(outputs):
    """``outputs``: {name: (float64 value, float64 sum of the magnitudes of its terms, den)}.  Asserts that every value is a multiple of
    ``1 / den`` and returns the largest ``sum of magnitudes * den / 2^24`` (exact in fp32 in any order where that is below 1)."""
    worst = 0.0
    for name, (value, terms, den) in outputs.items():
        scaled = value * den
        assert torch.equal(scaled, scaled.round()), f"{name}: not a multiple of 1/{den}"
        assert bool((terms >= value.abs()).all()), f"{name}: the magnitude sum does not bound the value"
        if terms.numel():
            worst = max(worst, float(terms.max()) * den / LIMIT)
    return worst


def _thinned(build, what):
    """The first of ``build(density)`` over DENSITIES whose outputs satisfy the exactness bound."""
    for density in DENSITIES:
        case = build(density)
        case.ratio = max(exactness(o) for o in case.exact.values())
        if case.ratio < 1.0:
            case.density = density
            return case
    raise AssertionError(f"{what}: no gradient density down to {DENSITIES[-1]} keeps the sums exact in fp32")


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1_000_003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _choice(g, shape, values):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=g)]


def _elu_grad(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def _mask(n, width):
    """The dropout factors ({0, 2}) of rows ``row0 .. row0 + n`` at DROP."""
    from pathpyg_amd.nn.sharded import dropout_mask
    p, seed, tag, row0 = DROP
    return dropout_mask(torch.arange(row0, row0 + n), width, p, seed, tag).double()


# ---------------------------------------------------------------------------------------------------------------- graph
@functools.lru_cache(maxsize=None)
def graph(n, n_src, degree):
    """A random row-sorted CSR of ``n`` rows over ``n_src`` columns with ``degree * n`` random entries and, in the last three rows (the
    last tile of the last pass; at 8 R + 1 rows that tile holds the long row alone and the other two end the tile before it): row n - 1
    with LONG_ROW entries, row n - 2 empty, row n - 3 with neighbours in the first tile only.  Row 5 (tile 0) is the second long row.  ``degree`` 4 keeps nnz <= 8 n (the register-capped backward kernel), 12 does not."""
    g = _gen(n, n_src, degree)
    row = torch.randint(0, n, (degree * n,), generator=g)
    idx = torch.randint(0, n_src, (degree * n,), generator=g)
    special = (row == n - 1) | (row == n - 2) | (row == n - 3) | (row == 5)
    row, idx = row[~special], idx[~special]
    near = min(16, n_src)
    row = torch.cat((row, torch.full((LONG_ROW,), n - 1), torch.full((LONG_ROW,), 5), torch.full((6,), n - 3)))
    idx = torch.cat((idx, torch.randint(0, n_src, (2 * LONG_ROW,), generator=g), torch.randint(0, near, (6,), generator=g)))
    order = torch.sort(row, stable=True).indices
    row, idx = row[order], idx[order]
    e = row.numel()
    assert (e <= 8 * n) == (degree == 4)
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    assert int(ptr[n - 1] - ptr[n - 2]) == 0 and int(ptr[n] - ptr[n - 1]) == LONG_ROW and int(ptr[6] - ptr[5]) == LONG_ROW
    val = _choice(g, (e,), (0.5, 1.0, 1.5))
    gr = types.SimpleNamespace(n=n, n_src=n_src, nnz=e, ptr=ptr.int(), idx=idx.int(), val=val, _coo={})

    def matrix(weighted):
        """The float64 sparse matrix of the CSR, with its values or with ones."""
        if weighted not in gr._coo:
            gr._coo[weighted] = torch.sparse_coo_tensor(torch.stack((row, idx)), val if weighted else torch.ones_like(val), (n, n_src)).coalesce()
        return gr._coo[weighted]

    gr.matrix = matrix
    return gr


# ---------------------------------------------------------------------------------------------------------------- gcn_forward
# rows per loop step of a workgroup (R): k_gcn_forward runs kGcnThreads / kWave = 4 waves (8 at the 128-wide shapes: 512 threads) of one
# 16-row tile each; k_wide_layer kWideWaves = 4 waves of 16 rows; k_wide_ws one kWsTile = 64-row tile
FORWARD_SHAPES = {(64, 64): 64, (16, 32): 64, (32, 16): 64, (128, 128): 128, (64, 128): 128, (128, 64): 128,
                  (64, 256): 64, (256, 64): 64, (128, 256): 64, (256, 128): 64, (256, 256): 64}
# more_sources: x has 1.5 n rows and idx reaches them; drop only where gcn_drop_supported (not with a side of 256)
FORWARD_VARIANTS = {
    "plain": dict(self=True, val=True, agg=True, heavy=False, drop=False, more_sources=True, degree=4),
    "bare": dict(self=False, val=False, agg=False, heavy=False, drop=False, more_sources=False, degree=12),
    "heavy": dict(self=True, val=True, agg=True, heavy=True, drop=False, more_sources=True, degree=4),
    "drop": dict(self=True, val=True, agg=False, heavy=False, drop=True, more_sources=True, degree=4),
}


def forward_case(p, q, n, variant):
    """``agg = A x + diag(self) x``, ``y = agg W^T + b`` (times the dropout factors): exact; ``y_elu = ELU(agg W^T + b)`` (times them)."""
    v = FORWARD_VARIANTS[variant]
    n_src = n + n // 2 if v["more_sources"] else n
    gr = graph(n, n_src, v["degree"])
    g = _gen(p, q, n, 1)
    x, w, bias = _ints(g, (n + n // 2, p), -2, 2)[:n_src], _choice(g, (q, p), WEIGHTS), _ints(g, (q,), -4, 4) / 4
    sc = _ints(g, (n,), 0, 4) / 4 if v["self"] else None
    a = gr.matrix(v["val"])
    factor = _mask(n, q) if v["drop"] else 1.0

    def run(x_, w_, b_):
        agg = torch.sparse.mm(a, x_)
        if sc is not None:
            agg += sc.unsqueeze(1) * x_[:n]
        return agg, agg @ w_.t() + b_

    (agg, pre), (agg_terms, pre_terms) = run(x, w, bias), run(x.abs(), w.abs(), bias.abs())
    case = types.SimpleNamespace(graph=gr, n=n, x=x, w=w, bias=bias, self_coef=sc, use_val=v["val"], want_agg=v["agg"], heavy=v["heavy"],
                                 drop=DROP if v["drop"] else None, y_elu=F.elu(pre) * factor,
                                 exact={"forward": {"agg": (agg, agg_terms, 4), "y": (pre * factor, pre_terms * factor, 8)}})
    case.ratio = exactness(case.exact["forward"])
    assert case.ratio < 1.0, f"forward {p}x{q} n={n} {variant}: ratio {case.ratio} to 2^24"
    return case


# ---------------------------------------------------------------------------------------------------------------- the backward kernels
def _gcn_gradients(a, n, n_self, dpre, sc, w, factor, x_in, agg_below):
    """G = A dpre + diag(self) dpre (rows below n_self), d_in = (G W) * factor, its column sums, dW = G^T x_in, dW_below = d_in^T agg_below;
    each with the sum of its terms' magnitudes (``factor`` >= 0)."""
    def run(d_, w_, x_, below_):
        gmat = torch.sparse.mm(a, d_)
        gmat[:n_self] += sc[:n_self].unsqueeze(1) * d_[:n_self]
        d_in = (gmat @ w_) * factor
        out = {"d_in": d_in, "colsum": d_in.sum(0)}
        if x_ is not None:
            out["dw"] = gmat.t() @ x_
        if below_ is not None:
            out["dw_below"] = d_in.t() @ below_
        return out

    absolute = lambda t: None if t is None else t.abs()
    value, terms = run(dpre, w, x_in, agg_below), run(dpre.abs(), w.abs(), absolute(x_in), absolute(agg_below))
    den = {"d_in": 16, "colsum": 16, "dw": 8, "dw_below": 16}       # G: 1/4; W: 1/2; ELU': 1/2; stored activations: 1/2; aggregates: integers
    return {name: (value[name], terms[name], den[name]) for name in value}


# k_gcn_backward: kGcnWaves = 4 waves of one 16-row tile per loop step (R = 64); both graphs: degree 4 -> register-capped kernel
# (except with heavy rows / dropout, which have no capped variant), degree 12 -> the 2-wave kernel
BACKWARD_SHAPES = {(64, 64): 64, (16, 64): 64, (64, 32): 64}
BACKWARD_VARIANTS = {
    "fuse": dict(fuse=True, shard=False, heavy=False, drop=False),
    "linear": dict(fuse=False, shard=False, heavy=False, drop=False),
    "shard": dict(fuse=True, shard=True, heavy=False, drop=False),           # n_self = 3 n / 4, dpre of n_self rows
    "heavy": dict(fuse=True, shard=False, heavy=True, drop=False),
    "drop": dict(fuse=True, shard=False, heavy=False, drop=True),
}
# gcn_input_grad: the 128-wide k_gcn_forward (8 waves, R = 128) and the 256-sided k_wide_layer / k_wide_ws (R = 64), kEpi == 1
INPUT_GRAD_SHAPES = {(128, 128): 128, (64, 128): 128, (128, 64): 128, (64, 256): 64, (256, 64): 64, (128, 256): 64, (256, 128): 64, (256, 256): 64}
INPUT_GRAD_VARIANTS = dict(BACKWARD_VARIANTS)                               # "linear": x_act None; "drop" only at the 128-wide shapes


def backward_case(m, k, n, degree, variant, below=False):
    """Inputs and exact results of gcn_backward / gcn_input_grad (``dw`` unused there) / gcn_backward_below on the source-major CSR."""
    v = BACKWARD_VARIANTS[variant]
    n_self = 3 * n // 4 if v["shard"] else n
    gr = graph(n, n_self, degree)
    g = _gen(m, k, n, degree, 2)
    x, w, sc = _choice(g, (n, k), (-0.5, 1.0)), _choice(g, (m, k), WEIGHTS), _ints(g, (n,), 0, 4) / 4
    agg_below = _ints(g, (n, 64), -2, 2) if below else None
    x_in = x * _mask(n, k) if v["drop"] else x                               # the kernels read the DROPPED activation: {-1, 0, 2}
    # ELU' from what is stored: at the activation itself, i.e. the stored value times 1 - p under dropout (1 at a dropped entry, times 0)
    factor = (_mask(n, k) if v["drop"] else 1.0) * _elu_grad(x) if v["fuse"] else torch.ones_like(x)
    gd = _gen(m, k, n, degree, 3)
    raw, keep = _choice(gd, (n_self, m), (-1.0, 1.0)), torch.rand((n_self, m), generator=gd)

    def build(density):
        dpre = raw * (keep < density)
        return types.SimpleNamespace(graph=gr, n=n, n_self=n_self, dpre=dpre, self_coef=sc, x=x_in, w=w, fuse=v["fuse"], heavy=v["heavy"],
                                     drop=DROP if v["drop"] else None, agg_below=agg_below,
                                     exact={"backward": _gcn_gradients(gr.matrix(True), n, n_self, dpre, sc, w, factor, x_in, agg_below)})

    return _thinned(build, f"backward {m}x{k} n={n} degree {degree} {variant}")


# ---------------------------------------------------------------------------------------------------------------- the head
HEAD_ROWS = 64                                        # k_head_forward / k_head_backward: kWavesPerBlock = 4 waves of one 16-row tile
HEAD_WIDTHS = [(64, 64, 64), (16, 32, 64), (32, 16, 16)]
HEAD_CLASSES = [2, 16]


def head_case(ha, hx, hb, c, n):
    """Inputs of head_forward (``z``, ``logits``: float64, compared at 1e-5) and the exact gradients of head_backward for a STORED ``z_in``
    in {-1/2, 1}: the formulas of tests/test_gpu_head_fused.py."""
    g = _gen(ha, hx, hb, c, n, 4)
    agg, x, deg = _ints(g, (n, ha), -2, 2), _choice(g, (n, hx), (-0.5, 1.0)), _ints(g, (n,), 0, 3)
    deg[::3] = 0.0
    w1, w2, wlin = _choice(g, (hb, ha), WEIGHTS), _choice(g, (hb, hx), WEIGHTS), _choice(g, (c, hb), WEIGHTS)
    b1, b2, blin = _ints(g, (hb,), -4, 4) / 4, _ints(g, (hb,), -4, 4) / 4, _ints(g, (c,), -4, 4) / 4
    z_in = _choice(g, (n, hb), (-0.5, 1.0))
    # the forward pass with agg, w2, b1 and b2 an eighth the size (``forward``): most pre-activations stay where ELU is neither saturated nor linear
    forward = {"agg": agg / 8, "w2": w2 / 8, "b1": b1 / 8, "b2": b2 / 8}
    pre = forward["agg"] @ w1.t() + deg.unsqueeze(1) * (x @ forward["w2"].t() + forward["b2"] + forward["b1"])
    z = torch.where(pre > 0, pre, torch.expm1(pre))
    raw, keep = _choice(g, (n, c), (-1.0, 1.0)), torch.rand((n, c), generator=g)
    fz, fx = _elu_grad(z_in), _elu_grad(x)

    def gradients(dl, w1_, w2_, wlin_, agg_, x_, z_):
        dpre = (dl @ wlin_) * fz
        dper = deg.unsqueeze(1) * dpre
        dpre_fo = (dper @ w2_) * fx
        return {"d_agg": dpre @ w1_, "dpre_fo": dpre_fo, "colsum_fo": dpre_fo.sum(0), "dW1": dpre.t() @ agg_, "dW2": dper.t() @ x_,
                "db1": dper.sum(0), "db2": dper.sum(0), "dWlin": dl.t() @ z_, "dblin": dl.sum(0)}

    den = {"d_agg": 8, "dpre_fo": 16, "colsum_fo": 16, "dW1": 4, "dW2": 8, "db1": 4, "db2": 4, "dWlin": 2, "dblin": 1}

    def build(density):
        dl = raw * (keep < density)
        value, terms = gradients(dl, w1, w2, wlin, agg, x, z_in), gradients(dl.abs(), w1.abs(), w2.abs(), wlin.abs(), agg.abs(), x.abs(), z_in.abs())
        return types.SimpleNamespace(n=n, agg=agg, x=x, deg=deg, w1=w1, b1=b1, w2=w2, b2=b2, wlin=wlin, blin=blin, z_in=z_in, dlogits=dl,
                                     forward=forward, z=z, logits=z @ wlin.t() + blin,
                                     exact={"backward": {name: (value[name], terms[name], den[name]) for name in value}})

    return _thinned(build, f"head {ha}/{hx}/{hb} C={c} n={n}")


# ---------------------------------------------------------------------------------------------------------------- dense
# k_dense_lds, the shapes with dense_supported == 3: ROWS = 16 * RT * (16 / (Q / 64)) rows per workgroup and loop step = 256 (Q = 64),
# 128 (Q = 128), 64 * kGemmRowTiles = 128 (Q = 256)
DENSE_SHAPES = {(64, 128): 128, (64, 256): 128, (128, 64): 256, (128, 128): 128, (128, 256): 128, (256, 64): 256, (256, 128): 128, (256, 256): 128}


def dense_case(p, q, n):
    """``out = a W + b`` (forward layout) and ``grad = (d W) * ELU'(y)`` with its column sums (gradient layout); ``W`` is [p, q]: the test hands
    it over as it is or transposed."""
    g = _gen(p, q, n, 5)
    a, w, bias, y = _ints(g, (n, p), -2, 2), _choice(g, (p, q), WEIGHTS), _ints(g, (q,), -4, 4) / 4, _choice(g, (n, q), (-0.5, 1.0))
    raw, keep = _choice(g, (n, p), (-1.0, 1.0)), torch.rand((n, p), generator=g)
    fy = _elu_grad(y)

    def build(density):
        d = raw * (keep < density)
        grad, grad_terms = (d @ w) * fy, (d.abs() @ w.abs()) * fy
        return types.SimpleNamespace(n=n, a=a, w=w, bias=bias, y=y, d=d, exact={
            "forward": {"out": (a @ w + bias, a.abs() @ w.abs() + bias.abs(), 4)},
            "gradient": {"grad": (grad, grad_terms, 4), "colsum": (grad.sum(0), grad_terms.sum(0), 4)}})

    return _thinned(build, f"dense {p}x{q} n={n}")


def all_cases():
    """(id, thunk) of every case the GPU module runs: what the host-side exactness test walks."""
    for (p, q), r in FORWARD_SHAPES.items():
        for n in row_counts(r):
            for variant in FORWARD_VARIANTS:
                yield f"forward-{p}x{q}-{n}-{variant}", functools.partial(forward_case, p, q, n, variant)
    for (m, k), r in BACKWARD_SHAPES.items():
        for degree in (4, 12):
            for n in row_counts(r):
                for variant in BACKWARD_VARIANTS:
                    yield f"backward-{m}x{k}-d{degree}-{n}-{variant}", functools.partial(backward_case, m, k, n, degree, variant)
    for n in row_counts(64):
        yield f"below-{n}", functools.partial(backward_case, 64, 64, n, 4, "fuse", True)
    for (m, k), r in INPUT_GRAD_SHAPES.items():
        for n in row_counts(r):
            for variant in INPUT_GRAD_VARIANTS:
                yield f"input_grad-{m}x{k}-{n}-{variant}", functools.partial(backward_case, m, k, n, 4, variant)
    for widths in HEAD_WIDTHS:
        for c in HEAD_CLASSES:
            for n in row_counts(HEAD_ROWS):
                yield f"head-{widths}-{c}-{n}", functools.partial(head_case, *widths, c, n)
    for (p, q), r in DENSE_SHAPES.items():
        for n in row_counts(r):
            yield f"dense-{p}x{q}-{n}", functools.partial(dense_case, p, q, n)
