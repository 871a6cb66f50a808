"""Inputs and float64 references of tests/test_gpu_value_domain.py: what the kernels do to VALUES at the ends of the fp32 range.

Plain torch-CPU code (no GPU, no library call): tests/test_host_logic.py runs the builders and their exactness condition where no GPU
is present.

ELU / ELU'.  ``ELU_X`` holds fp32 pre-activations on every branch of ``elu_fast`` (csrc/pp_common.h: the polynomial on (-0.25, 0], the
exponential below, the identity above 0) and ``ACT_GRID`` stored activations for ``ELU'(y) = y > 0 ? 1 : y + 1``.  The builders give,
per kernel family, inputs for which everything IN FRONT of the epilogue is exact in fp32: a CSR row has one neighbour of coefficient 1 and
no self term, or the self term alone with coefficient 1; a weight matrix holds a single 1.0 per output column (a selection); biases are
zero; the head runs once with ``deg = 0`` (``pre = agg``) and once with ``deg = 1, agg = 0`` (``pre = x``); upstream gradients are powers
of two; dropout runs at p = 1/2.  Every sum in front of the epilogue then has ONE non-zero term, which is the grid value itself (times a
power of two): the kernel's output isolates its epilogue, and ``front(torch.float32) == front(torch.float64)`` proves it on the CPU.
The grids have a length coprime to every width in use and are laid out row-major in a cycle, so with at least ``len(grid)`` rows every
value appears in every column — every column residue of a 16-wide tile, both halves of a packed pair.

Cross-entropy and Adam.  ``cross_entropy_reference`` is ``F.cross_entropy`` on the float64 logits with its autograd gradient and
``adam_reference`` a plain float64 restatement of torch.optim.Adam; the host test holds the first to the formula written out
(``cross_entropy_plain``) and the second to a float64 ``torch.optim.Adam``.
"""
import functools
import math
import types

import torch
import torch.nn.functional as F

F32 = torch.float32
TINY = 2.0 ** -126                                    # the smallest positive normal fp32 number
DROP = (0.5, 20240229, 33, 2 ** 33 + 11)              # (p, seed, tag, row0): 1 / (1 - p) = 2 and 1 - p = 1/2 are exact; global rows beyond 32 bits
WIDTHS = (7, 8, 16, 20, 32, 64, 128, 256)             # every matrix width in use: the grids' lengths are coprime to all of them


def _nextafter(x, towards):
    return float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(towards, dtype=F32)))


def _coprime_length(values):
    """``values`` (a list of floats) with its last entry repeated until the length is coprime to every width."""
    while any(math.gcd(len(values), w) != 1 for w in WIDTHS):
        values.append(values[-1])
    return torch.tensor(values, dtype=torch.float64).to(F32)


def elu_reference(x):
    """float64 ELU of an fp32 (or float64) tensor: x above 0, expm1(x) otherwise (signed zeros kept)."""
    x = x.double()
    return torch.where(x > 0, x, torch.expm1(x))


def elu_grad_reference(y):
    """float64 ELU' recovered from the stored activation: 1 above 0, y + 1 otherwise."""
    y = y.double()
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def _elu_inputs():
    quarter = -0.25
    named = [0.0, -0.0, 2.0 ** -100, -(2.0 ** -100), -1e-8, -1e-4, -1e-2, quarter, _nextafter(quarter, 0.0), _nextafter(quarter, -1.0),
             -0.5, -1.0, -5.0, -20.0, -100.0, 1e-4, 1.0, 100.0]
    spaced = (-torch.logspace(-20.0, math.log2(88.0), 200, base=2.0, dtype=torch.float64)).to(F32).tolist()
    x = _coprime_length(named + spaced)
    assert bool(torch.isfinite(x).all()) and bool(((x == 0) | (x.abs() >= TINY)).all())          # no subnormals, nothing non-finite
    return x


ELU_X = _elu_inputs()                                 # fp32 pre-activations
ELU_GRID = (ELU_X, elu_reference(ELU_X))              # ... with their float64 ELU values


def _activations():
    images = elu_reference(ELU_X).to(F32)             # what a correctly rounded ELU stores
    images = images[(images == 0) | (images.abs() >= TINY)].tolist()
    return _coprime_length(images + [-1.0, -1.0 + 2.0 ** -24, -0.0, 0.0, TINY])


ACT_GRID = _activations()                             # fp32 stored activations (ELU' = y > 0 ? 1 : y + 1)


def lay_out(grid, n, width, shift=0):
    """[n, width] fp32: ``grid`` cycled row-major.  The length of the grid is coprime to ``width``, so from ``len(grid)`` rows on every
    value stands in every column."""
    assert math.gcd(len(grid), width) == 1 and n >= len(grid)
    return grid[(torch.arange(n * width) + shift) % len(grid)].reshape(n, width).clone()


def covers(matrix, grid):
    """Whether every column of ``matrix`` holds every value of ``grid`` (a sum in front of an epilogue may turn -0.0 into 0.0: one value)."""
    want = (grid + 0.0).unique()
    return all(bool(torch.isin(want, matrix[:, c] + 0.0).all()) for c in range(matrix.size(1)))


def selection(q, p, offset=0):
    """W [q, p] (Linear layout: ``y = x W^T``) with one 1.0 per output: output column j reads input column (j * max(1, p // q) + offset) % p."""
    w = torch.zeros(q, p, dtype=F32)
    w[torch.arange(q), (torch.arange(q) * max(1, p // q) + offset) % p] = 1.0
    return w


def selected(q, p, offset=0):
    """The input column behind every output column of ``selection(q, p, offset)``."""
    return (torch.arange(q) * max(1, p // q) + offset) % p


def powers_of_two(shape, seed):
    """Upstream gradients: +-2^e, e in [-6, 6] — a product with any fp32 number above 2^-100 in magnitude is exact."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-6, 7, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (sign * torch.pow(2.0, e.double())).to(F32)


def drop_factors(n, width):
    """The dropout factors ({0, 2}) of rows ``row0 .. row0 + n`` at DROP."""
    from pathpyg_amd.nn.sharded import dropout_mask
    p, seed, tag, row0 = DROP
    return dropout_mask(torch.arange(row0, row0 + n), width, p, seed, tag).to(F32)


# ---------------------------------------------------------------------------------------------------------------- CSR rows
def csr(n, style):
    """``neighbour``: row r has the one neighbour (r + 37) % n with coefficient 1 and a self coefficient of 0;  ``self``: empty rows, self
    coefficient 1.  Returns (ptr int32 [n + 1], idx int32, val fp32, self_coef fp32 [n], source row of every output row)."""
    if style == "neighbour":
        src = (torch.arange(n) + 37) % n
        return torch.arange(n + 1, dtype=torch.int32), src.int(), torch.ones(n, dtype=F32), torch.zeros(n, dtype=F32), src
    assert style == "self"
    # (16 entries that no row owns: the arrays of an empty CSR are still real allocations, as a plan builder hands them out)
    return torch.zeros(n + 1, dtype=torch.int32), torch.zeros(16, dtype=torch.int32), torch.zeros(16, dtype=F32), torch.ones(n, dtype=F32), torch.arange(n)


def _aggregate(x, src, val_one, self_coef):
    """A x + diag(self) x of a ``csr`` in the dtype of ``x``: one neighbour (coefficient ``val_one``) and the self term."""
    return x[src] * val_one + self_coef.to(x.dtype).unsqueeze(1) * x[: src.numel()]


# ---------------------------------------------------------------------------------------------------------------- forward builders
def spmm_case(n, f, style):
    """pp_spmm_f32 with act = 1: ``pre = x[source row]`` (a zero bias is added)."""
    ptr, idx, val, sc, src = csr(n, style)
    x, bias = lay_out(ELU_X, n, f), torch.zeros(f, dtype=F32)
    neighbour = 1.0 if style == "neighbour" else 0.0
    front = lambda dt: _aggregate(x.to(dt), src, neighbour, sc) + bias.to(dt)
    return types.SimpleNamespace(n=n, ptr=ptr, idx=idx, val=val, self_coef=sc, x=x, bias=bias, front=front, pre=front(F32), grid=ELU_X)


def gcn_forward_case(n, p, q, style, offset=0):
    """pp_gcn_forward(_drop)_f32 / pp_wide_layer_f32 epilogue 0: ``pre[r, j] = x[source row, selected column of j]``."""
    ptr, idx, val, sc, src = csr(n, style)
    x, w, bias = lay_out(ELU_X, n, p), selection(q, p, offset), torch.zeros(q, dtype=F32)
    neighbour = 1.0 if style == "neighbour" else 0.0
    front = lambda dt: _aggregate(x.to(dt), src, neighbour, sc) @ w.to(dt).t() + bias.to(dt)
    return types.SimpleNamespace(n=n, ptr=ptr, idx=idx, val=val, self_coef=sc, x=x, w=w, bias=bias, front=front, pre=front(F32), grid=ELU_X)


def bip_combine_case(n, f, which):
    """pp_bip_combine_f32, ``ELU(A + deg (P + bias))``:  ``a``: deg = 0, pre = A (P holds finite numbers);  ``p``: deg = 1, A = 0, pre = P."""
    grid, other = lay_out(ELU_X, n, f), lay_out(ELU_X, n, f, shift=5)
    bias = torch.zeros(f, dtype=F32)
    if which == "a":
        a, p, deg = grid, other, torch.zeros(n, dtype=F32)
    else:
        a, p, deg = torch.zeros(n, f, dtype=F32), grid, torch.ones(n, dtype=F32)
    front = lambda dt: a.to(dt) + deg.to(dt).unsqueeze(1) * (p.to(dt) + bias.to(dt))
    return types.SimpleNamespace(n=n, a=a, p=p, deg=deg, bias=bias, front=front, pre=front(F32), grid=ELU_X)


def head_forward_case(n, ha, hx, hb, c, which, offset=0):
    """pp_dbgnn_head_forward_f32, ``z = ELU(agg W1^T + deg (x W2^T + b2 + b1))``:  ``agg``: deg = 0 and W1 a selection, pre = agg[:, selected];
    ``x``: deg = 1, agg = 0, b1 = b2 = 0 and W2 a selection, pre = x[:, selected]."""
    g = torch.Generator().manual_seed(ha * 10000 + hx * 100 + hb + c)
    wlin, blin = torch.randn(c, hb, generator=g) / 8, torch.randn(c, generator=g)
    b1, b2 = torch.zeros(hb, dtype=F32), torch.zeros(hb, dtype=F32)
    if which == "agg":
        agg, x, deg = lay_out(ELU_X, n, ha), lay_out(ACT_GRID, n, hx), torch.zeros(n, dtype=F32)
        w1, w2 = selection(hb, ha, offset), torch.randn(hb, hx, generator=g)
    else:
        agg, x, deg = torch.zeros(n, ha, dtype=F32), lay_out(ELU_X, n, hx), torch.ones(n, dtype=F32)
        w1, w2 = torch.randn(hb, ha, generator=g), selection(hb, hx, offset)
    front = lambda dt: agg.to(dt) @ w1.to(dt).t() + deg.to(dt).unsqueeze(1) * (x.to(dt) @ w2.to(dt).t() + b2.to(dt) + b1.to(dt))
    return types.SimpleNamespace(n=n, agg=agg, x=x, deg=deg, w1=w1, b1=b1, w2=w2, b2=b2, wlin=wlin, blin=blin, front=front, pre=front(F32), grid=ELU_X)


# ---------------------------------------------------------------------------------------------------------------- backward builders
def elementwise_case(n, f, seed, dropped=False):
    """pp_act_backward_f32, pp_bip_combine_backward_f32, pp_dropout_act_backward_f32: ``g`` powers of two, ``y`` the activations (stored
    dropped — times the factor in {0, 2} — when ``dropped``).  ``front`` is the upstream gradient itself."""
    g, act = powers_of_two((n, f), seed), lay_out(ACT_GRID, n, f)
    factor = drop_factors(n, f) if dropped else None
    front = lambda dt: g.to(dt)
    return types.SimpleNamespace(n=n, g=g, act=act, y=act * factor if dropped else act, factor=factor, front=front, pre=g, grid=ACT_GRID,
                                 deg=torch.pow(2.0, (torch.arange(n) % 3).double()).to(F32))


def gradient_case(n, m, k, seed, style="neighbour", dropped=False, offset=0):
    """The gradient epilogues behind a product: ``front[r, j] = d[source row, selected column of j]`` with d [n, m] powers of two, the
    weight [m, k] a selection (one 1.0 per output column j), ``act`` [n, k] the stored activations (``y``: as the kernel reads them, dropped
    when ``dropped``).  Serves pp_dense_f32 / pp_dense_narrow_f32 (grad_act; style ``self``: no graph), pp_dense_backward_f32, the
    pp_gcn_backward_* family, pp_gcn_input_grad_f32 / pp_wide_layer_f32 epilogue 1 and pp_spmm_act_backward(_drop)_f32 (m == k, identity)."""
    ptr, idx, val, sc, src = csr(n, style)
    d, w, act = powers_of_two((n, m), seed), selection(k, m, offset).t().contiguous(), lay_out(ACT_GRID, n, k)
    factor = drop_factors(n, k) if dropped else None
    neighbour = 1.0 if style == "neighbour" else 0.0
    front = lambda dt: _aggregate(d.to(dt), src, neighbour, sc) @ w.to(dt)
    return types.SimpleNamespace(n=n, ptr=ptr, idx=idx, val=val, self_coef=sc, d=d, w=w, act=act, y=act * factor if dropped else act, factor=factor,
                                 front=front, pre=front(F32), grid=ACT_GRID)


def head_backward_case(n, ha, hx, hb, c, which, offset=0):
    """pp_dbgnn_head_backward_f32 with deg in {1, 2, 4}, dlogits powers of two, Wlin [c, hb] a selection (dz[:, j] = dlogits[:, j % c]):
    ``z``: z the activations, x = 1, W1 [hb, ha] a selection — d_agg[r, j] = dz[r, s(j)] ELU'(z[r, s(j)]) (deg must NOT enter);
    ``x``: z = 1, x the activations, W2 [hb, hx] a selection — dpre_fo[r, j] = deg[r] dz[r, s(j)] ELU'(x[r, j])."""
    g = torch.Generator().manual_seed(ha * 10000 + hx * 100 + hb + c + 1)
    dl, wlin = powers_of_two((n, c), ha + hx + hb + c), selection(hb, c).t().contiguous()
    deg, agg = torch.pow(2.0, (torch.arange(n) % 3).double()).to(F32), torch.randn(n, ha, generator=g)
    dz = lambda dt: dl.to(dt) @ wlin.to(dt)
    if which == "z":
        z, x = lay_out(ACT_GRID, n, hb), torch.ones(n, hx, dtype=F32)
        w1, w2 = selection(ha, hb, offset).t().contiguous(), torch.randn(hb, hx, generator=g)
        front = lambda dt: dz(dt)[:, selected(ha, hb, offset)]                  # times ELU'(z) at the same columns, then W1: one term per output
        act = z[:, selected(ha, hb, offset)]
    else:
        z, x = torch.ones(n, hb, dtype=F32), lay_out(ACT_GRID, n, hx)
        w1, w2 = torch.randn(hb, ha, generator=g), selection(hx, hb, offset).t().contiguous()
        front = lambda dt: (deg.to(dt).unsqueeze(1) * dz(dt)) @ w2.to(dt)
        act = x
    return types.SimpleNamespace(n=n, dlogits=dl, z=z, agg=agg, x=x, deg=deg, w1=w1, w2=w2, wlin=wlin, act=act, front=front, pre=front(F32), grid=ACT_GRID)


FORWARD_SHAPES = [(16, 16), (32, 64), (64, 64), (128, 128), (64, 128), (256, 256), (64, 256), (256, 64)]
HEAD_WIDTHS = [(64, 64, 64), (16, 32, 64)]
GRADIENT_SHAPES = [((64, 64), "neighbour"), ((64, 64), "self"), ((8, 64), "self"), ((16, 32), "self"), ((128, 128), "neighbour"),
                   ((256, 256), "neighbour"), ((16, 64), "neighbour"), ((64, 32), "neighbour")]


def all_cases():
    """(id, thunk, whether every value must stand in every column) of the builders as tests/test_gpu_value_domain.py calls them."""
    part = functools.partial
    for f in (64, 7):
        for style in ("neighbour", "self"):
            yield f"spmm-{f}-{style}", part(spmm_case, 512, f, style), True
    for p, q in FORWARD_SHAPES:
        for style in ("neighbour", "self"):
            yield f"gcn_forward-{p}x{q}-{style}", part(gcn_forward_case, 512, p, q, style), True
    for f in (64, 20):
        for which in ("a", "p"):
            yield f"bip_combine-{f}-{which}", part(bip_combine_case, 512, f, which), True
    for widths in HEAD_WIDTHS:
        for which in ("agg", "x"):
            yield f"head_forward-{widths}-{which}", part(head_forward_case, 512, *widths, 8, which), True
        for which in ("z", "x"):
            yield f"head_backward-{widths}-{which}", part(head_backward_case, 512, *widths, 8, which), True
    for f in (64, 7):
        yield f"elementwise-{f}", part(elementwise_case, 512, f, 3), True
    yield "elementwise-dropped", part(elementwise_case, 1024, 64, 4, True), False
    for (m, k), style in GRADIENT_SHAPES:
        yield f"gradient-{m}x{k}-{style}", part(gradient_case, 512, m, k, m + k, style), True
    yield "gradient-dropped", part(gradient_case, 1024, 64, 64, 5, "neighbour", True), False


# ---------------------------------------------------------------------------------------------------------------- cross-entropy
def cross_entropy_reference(logits, target):
    """(mean loss, d loss / d logits) in float64 from fp32 logits [n, C] (-inf allowed) and int64 targets: ``F.cross_entropy`` on the
    float64 logits with its autograd gradient."""
    leaf = logits.double().requires_grad_(True)
    loss = F.cross_entropy(leaf, target)
    loss.backward()
    return loss.detach(), leaf.grad


def cross_entropy_plain(logits, target):
    """The same two numbers written out in float64 — (m - z[y]) + log1p(sum over c != argmax of exp(z[c] - m)) per row, softmax minus
    one-hot over n — for the host test to hold ``cross_entropy_reference`` against.  On a row whose target leads by 20 the loss is 4e-8
    and F.cross_entropy's ``z[y] - m - log(sum)`` carries half an ulp of 20 (2e-15): the two agree to 1e-7 there, to 1e-12 elsewhere."""
    z = logits.double()
    n = z.size(0)
    m, first = z.max(1, keepdim=True)
    e = torch.exp(z - m)
    rows = torch.arange(n)
    rest = e.clone()
    rest[rows, first.squeeze(1)] = 0.0
    loss = (m.squeeze(1) - z[rows, target]) + torch.log1p(rest.sum(1))
    grad = e / e.sum(1, keepdim=True)
    grad[rows, target] -= 1.0
    return loss.mean(), grad / n


CE_CLASSES = (2, 8, 13, 64)                           # k_cross_entropy<8>, <8>, <16>, <64>
CE_KINDS = ("spread40", "spread200", "margin12", "margin20", "masked", "masked_target")


def cross_entropy_case(kind, n, c):
    """fp32 logits [n, c] and targets:  ``spread*``: randn * 40 / * 200;  ``margin*``: randn with the target class raised by 12 / 20;
    ``masked``: randn * 3 with -inf in three of ten non-target entries;  ``masked_target``: the same with the target of every 97th row masked."""
    g = torch.Generator().manual_seed(CE_KINDS.index(kind) * 1_000_003 + n * 101 + c)
    z, y = torch.randn(n, c, generator=g), torch.randint(0, c, (n,), generator=g)
    rows = torch.arange(n)
    if kind.startswith("spread"):
        z = z * float(kind[6:])
    elif kind.startswith("margin"):
        z[rows, y] += float(kind[6:])
    else:
        z = z * 3
        hide = torch.rand(n, c, generator=g) < 0.3
        hide[rows, y] = False
        if kind == "masked_target":
            hide[rows[::97]] = False                  # (the target alone: a row of -inf only has no loss at all)
            hide[rows[::97], y[::97]] = True
        z[hide] = -math.inf
    return z, y


# ---------------------------------------------------------------------------------------------------------------- Adam
ADAM = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
ADAM_SHAPES = [(64, 64), (64,), (5, 7, 3)]
ADAM_STEPS = 100


def adam_inputs():
    """(initial fp32 tensors, [step][tensor] fp32 gradients 0.5 + 0.1 randn) from one seeded generator: gradients of one sign, so that a
    constant rounded once too often moves every step the same way."""
    g = torch.Generator().manual_seed(1234)
    init = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    grads = [[0.5 + 0.1 * torch.randn(s, generator=g) for s in ADAM_SHAPES] for _ in range(ADAM_STEPS)]
    return init, grads


def adam_reference(init, grads, lr, betas, eps, weight_decay):
    """torch.optim.Adam's update (amsgrad off, L2 weight decay) in float64 on the fp32 inputs: the parameters after ``len(grads)`` steps."""
    b1, b2 = betas
    p = [t.double().clone() for t in init]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    for step, gs in enumerate(grads, 1):
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        for i, gr in enumerate(gs):
            gr = gr.double() + weight_decay * p[i]
            m[i] += (1.0 - b1) * (gr - m[i])
            v[i] = b2 * v[i] + (1.0 - b2) * gr * gr
            p[i] -= (lr / bc1) * (m[i] / (v[i].sqrt() / math.sqrt(bc2) + eps))
    return p
