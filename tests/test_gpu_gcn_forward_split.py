"""The 64 x 64 layer product of k_gcn_forward on split-bf16 MFMAs (PP_FWD_SPLIT, pathpyg_amd/csrc/pp_gcn_fused.hip).

An fp32 value is hi + mid + lo with three truncated bf16 values; the kernel keeps the six largest cross products of a (tile, W) pair and
runs the fp32 instructions of before on tiles (or a W) outside the exponent window 2^-40 <= |x| < 2^60.  Checked here: the split loses no
bit (identity / signed power-of-two permutation weights give back x exactly), the product holds the project's 1e-5 against float64 at
three scales, values at the ends of the fp32 range behave as a float32 evaluation does, and the kept aggregate A x is untouched."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.tolerance import assert_embeddings_close, gradient_rtol_needed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 15, 16, 17, 63, 64, 65, 1000]
FLT_MAX = 3.4028234663852886e38


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from pathpyg_amd import _hip
    return _hip


def _graph(n, g):
    """CSR with in-degrees 0 .. 12: empty rows and the <= 4, 5 - 8 and > 8 neighbour paths of the gather stage."""
    deg = torch.randint(0, 13, (n,), generator=g)
    if n >= 15:
        deg[:4] = torch.tensor([0, 4, 8, 12])
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(deg, 0).int()
    e = int(ptr[-1])
    idx = torch.randint(0, n, (e,), generator=g, dtype=torch.int32)
    val = torch.rand(e, generator=g) + 0.1
    return ptr, idx, val, torch.repeat_interleave(torch.arange(n), deg)


def _self_only(n):
    """No neighbours, every row its own self term with coefficient 1: tile = x."""
    return torch.zeros(n + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.ones(n)


def _aggregate64(n, dst, idx, val, sc, x):
    agg = torch.zeros(n, x.size(1), dtype=torch.float64)
    coef = val.double() if val is not None else torch.ones(idx.numel(), dtype=torch.float64)
    agg.index_add_(0, dst, coef.unsqueeze(1) * x.double()[idx.long()])
    if sc is not None:
        agg += sc.double().unsqueeze(1) * x.double()
    return agg


def _d(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("n", SIZES)
def test_split_loses_no_bit(hip, n):
    """W = identity, then a signed permutation scaled by powers of two: only hi(W) is non-zero, so y = lo(x) w + mid(x) w + hi(x) w, every
    partial sum exact.  A bit lost in hi / mid / lo, or a wrong (column, k) pair in the staged B operands, shows as inequality."""
    g = torch.Generator().manual_seed(100 + n)
    ptr, idx, sc = _self_only(n)
    x = torch.randn(n, 64, generator=g)
    y = hip.gcn_forward(_d(ptr), _d(idx), None, n, _d(x), _d(sc), torch.eye(64, device=DEV), None, False).cpu()
    assert torch.equal(y, x)
    perm = torch.randperm(64, generator=g)
    factor = torch.ldexp(torch.ones(64), torch.randint(-20, 21, (64,), generator=g)) * (torch.randint(0, 2, (64,), generator=g) * 2 - 1)
    w = torch.zeros(64, 64)
    w[torch.arange(64), perm] = factor
    y = hip.gcn_forward(_d(ptr), _d(idx), None, n, _d(x), _d(sc), _d(w), None, False).cpu()
    assert torch.equal(y, x[:, perm] * factor)


VARIANTS = [  # (val, self_coef, bias + ELU, want_agg)
    (True, True, True, False), (False, True, False, True), (True, False, True, True), (False, False, False, False),
    (True, True, False, True), (False, True, True, False),
]


@pytest.mark.parametrize("n", SIZES)
def test_product_against_float64(hip, n):
    """act((A x) W^T + b) against float64 at the project's 1e-5 (tests/tolerance.py), x and W at scales 1, 1e-3 and 1e3; the kept aggregate
    is the one the unchanged 64 x 32 instantiation of the same gather stage returns, bit for bit, and pp_spmm's within rounding."""
    g = torch.Generator().manual_seed(200 + n)
    ptr, idx, val, dst = _graph(n, g)
    needed = 0.0
    for scale, (with_val, with_self, with_bias_act, want_agg) in itertools.product((1.0, 1e-3, 1e3), VARIANTS):
        x = torch.randn(n, 64, generator=g) * scale
        w = torch.randn(64, 64, generator=g) / 8 * scale
        b = torch.randn(64, generator=g) * scale * scale if with_bias_act else None
        sc = torch.rand(n, generator=g) + 0.1 if with_self else None
        v = val if with_val else None
        agg = _aggregate64(n, dst, idx, v, sc, x)
        pre = agg @ w.double().t()
        want = F.elu(pre + b.double()) if with_bias_act else pre
        out = hip.gcn_forward(_d(ptr), _d(idx), _d(v), n, _d(x), _d(sc), _d(w), _d(b), with_bias_act, want_agg=want_agg)
        got = out[0] if want_agg else out
        what = f"n={n} scale={scale:g} val={with_val} self={with_self} bias+elu={with_bias_act}"
        needed = max(needed, gradient_rtol_needed(got, want))
        assert_embeddings_close(got, want, what=what)
        if want_agg:
            same_gather = hip.gcn_forward(_d(ptr), _d(idx), _d(v), n, _d(x), _d(sc), _d(w[:32].contiguous()), None, False, want_agg=True)[1]
            assert torch.equal(out[1], same_gather), what + ": kept aggregate changed"
            if sc is not None:
                assert_embeddings_close(out[1], hip.spmm(_d(ptr), _d(idx), _d(v), n, _d(x), _d(sc), _d(x)), what=what + " A x vs spmm")
            assert_embeddings_close(out[1], agg, what=what + " A x")
    print(f"[split] n={n}: gradient_rtol_needed {needed:.2e} (bound 1e-05)")


def _check_like_float32(got, want, what):
    """NaN at the same places, the same signed infinities, every row's finite entries within 1e-5 of the float32 evaluation (row by row:
    a row of 1e38 must not lend its rms to the others)."""
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what + ": NaN positions"
    inf_g, inf_w = torch.isinf(got), torch.isinf(want)
    assert torch.equal(inf_g, inf_w), what + ": infinity positions"
    assert torch.equal(got[inf_g], want[inf_w]), what + ": infinity signs"
    fin = torch.isfinite(want)
    for r in range(want.size(0)):
        assert_embeddings_close(got[r][fin[r]], want[r][fin[r]], what=f"{what}, row {r}")


@pytest.mark.parametrize("act", [False, True], ids=["linear", "bias+elu"])
def test_range_ends(hip, act):
    """Single rows holding +-0, values above the largest bf16 (3.39e38 .. FLT_MAX), 1e-30, a subnormal, +-inf and NaN, the tiles between them
    ordinary: a rounding split turns FLT_MAX into inf, a missing fallback loses the tiny values or spreads NaN."""
    g = torch.Generator().manual_seed(7)
    n = 150                                                       # 10 tiles, the special rows in tiles 0, 2, 3, 5, 6, 8, 9
    x = torch.randn(n, 64, generator=g)
    x[3, 5], x[3, 6], x[3, 40:48] = 0.0, -0.0, 0.0                # zeros: inside the window
    x[35, 7], x[35, 50] = FLT_MAX, -3.395e38                      # beyond the largest bf16 value; |w| <= 0.4 keeps the sums finite
    x[36, 0] = -FLT_MAX
    x[50, 9], x[50, 33] = 1e-30, -1e-30
    x[51] = torch.randn(64, generator=g) * 1e-30                  # a whole row of tiny values: its outputs are tiny, not zero
    x[85, 3], x[85, 60] = 1e-40, -1e-40                           # subnormal
    x[100, 11] = float("inf")
    x[101, 12], x[101, 13] = float("inf"), float("-inf")
    x[102, 63] = float("-inf")
    x[130, 31] = float("nan")
    x[149, 0] = float("nan")
    w = (torch.randn(64, 64, generator=g) / 8).clamp(-0.4, 0.4)
    w = torch.where(w.abs() < 1e-3, torch.full_like(w, 1e-3), w)  # no inf * (almost) 0
    b = torch.randn(64, generator=g) if act else None
    ptr, idx, sc = _self_only(n)
    want = x @ w.t()
    if act:
        want = F.elu(want + b)
    got = hip.gcn_forward(_d(ptr), _d(idx), None, n, _d(x), _d(sc), _d(w), _d(b), act).cpu()
    _check_like_float32(got, want, "special tiles")
    assert bool((got[51] != 0).all())
    # W itself outside the window (one subnormal, one huge entry): the whole workgroup on the fp32 instructions
    w2 = w.clone()
    w2[0, 0], w2[5, 9] = 1e-40, 1e20
    x2 = x.clone()
    x2[35], x2[36] = x[34], x[37]                                 # (no 3e38 * 1e20: an overflow whose place depends on the order of the sum)
    want = x2 @ w2.t()
    if act:
        want = F.elu(want + b)
    got = hip.gcn_forward(_d(ptr), _d(idx), None, n, _d(x2), _d(sc), _d(w2), _d(b), act).cpu()
    _check_like_float32(got, want, "W outside the window")
