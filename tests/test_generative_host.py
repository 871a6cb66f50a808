"""Host side of pathpyg_amd.algorithms.generative_models: the stream definition (tests/cpu_ops_generative.py) held to published Philox
answers, ``math.log2`` and binomial statistics; the host functions held to fixtures made from the reference's own functions
(tests/golden/generative_vectors.npz); refusals and corner results.  No GPU is touched.  The distribution checks run on the restatement
alone with fixed seeds: they are deterministic, each either passes forever or is a finding, and the remedy is never a different seed."""
import math
import pathlib
import random
import warnings

import numpy as np
import pytest

import cpu_ops_generative as ops
from pathpyg_amd.algorithms import generative_models as gm

GOLDEN = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "generative_vectors.npz", allow_pickle=False)


class Duck:
    def __init__(self, n, m, directed):
        self.n, self.m, self._directed = n, m, directed

    def is_directed(self):
        return self._directed


# ------------------------------------------------------------------ the generator
@pytest.mark.parametrize("ctr, key, expect", [
    ([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, expect):
    assert " ".join("%08x" % x for x in ops.philox(ctr, key)) == expect


def test_counter_layout():
    """index -> c0, c1; stream -> c2 and the low 24 bits of c3; the tag on top of c3; the seed is the key."""
    seed, tag, stream, index = 0x0123456789ABCDEF, 5, (0xABCDEF << 32) | 0x11223344, (0x55667788 << 32) | 0x99AABBCC
    r = ops.philox([0x99AABBCC, 0x55667788, 0x11223344, (5 << 24) | 0xABCDEF], [0x89ABCDEF, 0x01234567])
    assert ops.word(seed, tag, stream, index) == r[0] | (r[1] << 32)
    assert ops.word(seed + (1 << 32), tag, stream, index) != ops.word(seed, tag, stream, index)
    assert ops.word(-1, 1, 0, 0) == ops.word((1 << 64) - 1, 1, 0, 0)


def test_integer_log_bound():
    """|neglog2 / 2^40 - (-log2 v)| <= 2^-40 plus the rounding of math.log2 itself (2^-46 at values up to 63)."""
    rnd = random.Random(1)
    draws = [0, 1, 2, 3, (1 << 64) - 1, (1 << 64) - 2, (1 << 63), (1 << 63) - 1]
    while len(draws) < 20000:
        w = rnd.getrandbits(64)
        draws.append(w >> rnd.randrange(60) if rnd.random() < 0.2 else w)
    worst = 0.0
    for w in draws:
        v = (w >> 1) + 1
        exact = 63 - (math.log2(v) if v < (1 << 53) else math.log2(v >> 10) + 10)
        worst = max(worst, abs(ops.neglog2(w) / 2.0 ** 40 - exact))
    assert ops.neglog2((1 << 64) - 1) == 0 and ops.neglog2(0) == 63 << 40
    assert worst <= 2.0 ** -40 + 2.0 ** -45, worst


def test_skip_constants():
    assert gm.skip_constant(1.0) == 0 and gm.skip_constant(0.5) == 1 << 32
    assert gm.skip_constant(gm.MIN_P) < 1 << 62
    assert gm.chunk_log2(0.125) == 10 and gm.chunk_log2(1.0) == 7 and gm.chunk_log2(0.125, 1) == 3
    assert gm.rewire_threshold(0.5) == (1 << 63, False) and gm.rewire_threshold(1.0)[1] and gm.rewire_threshold(0.0) == (0, False)


def test_skip_constant_against_exact_logarithm():
    """c 2^32 = -2^32 / log2(1 - p) from a 60-digit decimal logarithm of the exact value of 1 - p; the float route may differ by the
    rounding of log1p, a division and a product (relative 2^-50 covers them), never by more."""
    from decimal import Decimal, getcontext
    from fractions import Fraction
    getcontext().prec = 60
    for p in (2.0 ** -30, 1e-9, 1e-3, 0.05, 0.125, 0.3, 0.9, 1 - 2.0 ** -20, 1 - 2.0 ** -53):
        q = Fraction(1) - Fraction(p)
        exact = -(Decimal(2) ** 32) * Decimal(2).ln() / (Decimal(q.numerator) / Decimal(q.denominator)).ln()
        got = gm.skip_constant(p)
        assert 0 < got < 1 << 63 and abs(Decimal(got) - exact) <= exact * Decimal(2) ** -50 + 1, (p, got, exact)
    for p, k in ((2.0 ** -30, 37), (1e-3, 17), (0.9, 8), (0.05, 12), (1.0 / 128, 14)):
        assert gm.chunk_log2(p) == k and 2 ** k * p >= 128 > 2 ** (k - 1) * p
    assert gm.rewire_threshold(0.25) == (1 << 62, False) and gm.rewire_threshold(2.0 ** -64) == (1, False)
    assert gm.rewire_threshold(0.1)[0] == int(Fraction(0.1) * 2 ** 64)


def test_slot_decode():
    slots = {0, 1, 2, (1 << 62) - 1, (1 << 62), (1 << 62) + 1}
    for r in list(range(1, 70)) + [1 << 16, (1 << 31) - 2, 3037000499]:
        t = r * (r - 1) // 2
        slots |= {max(t - 1, 0), t, t + 1, r * r - 1, r * r, r * r + 1}
    for s in sorted(slots):
        r, c = ops.decode(ops.STRICT, 0, s)
        assert 0 <= c < r and r * (r - 1) // 2 + c == s
        r, c = ops.decode(ops.DIAG, 0, s)
        assert 0 <= c <= r and r * (r + 1) // 2 + c == s
    for cols in (1, 7, (1 << 31) - 2):
        for s in (0, cols - 1, cols, cols * cols - 1, cols * (cols + 1) - 1):
            r, c = ops.decode(ops.RECT, cols, s)
            assert 0 <= c < cols and r * cols + c == s
            r, c = ops.decode(ops.NO_DIAG, cols, s)
            assert c != r and 0 <= c <= cols and r * cols + (c - (c > r)) == s
    assert [gm.slot_space(5, d, l) for d in (False, True) for l in (False, True)] == [ops.slot_space(5, d, l) for d in (False, True) for l in (False, True)]


# ------------------------------------------------------------------ distributions, on the restatement
def test_gnp_edge_counts_within_5_sigma():
    for n, p in [(300, 0.05), (2000, 0.001), (60, 0.9), (40, 1.0), (46, 0.125)]:
        N = n * (n - 1) // 2
        for seed in range(5):
            slots = [s for _, s in ops.region_slots(seed, [(N, p, ops.STRICT, 0, 0, 0)])]
            assert slots == sorted(set(slots)) and all(0 <= s < N for s in slots)
            sd = math.sqrt(N * p * (1 - p))
            assert abs(len(slots) - N * p) <= 5 * sd, (n, p, seed, len(slots))


def test_sbm_block_pair_counts_within_5_sigma():
    M = [[0.3, 0.02, 0.0], [0.02, 0.5, 1.0], [0.0, 1.0, 0.1]]
    rnd = random.Random(5)
    z = [rnd.randrange(3) for _ in range(150)]
    regions, perm = ops.sbm_regions(M, z)
    for seed in (11, 12):
        counts = [0] * len(regions)
        for i, _ in ops.region_slots(seed, regions):
            counts[i] += 1
        for (N, p, *_), got in zip(regions, counts):
            assert abs(got - N * p) <= 5 * math.sqrt(N * p * (1 - p)), (N, p, got)
        edges = ops.sbm(M, z, seed)
        assert all((v, u) in set(edges) for u, v in edges) and all(u != v for u, v in edges)
        assert not any(z[u] == 0 and z[v] == 2 for u, v in edges)
        assert sum(1 for u, v in edges if z[u] == 1 and z[v] == 2) == sum(1 for b in z if b == 1) * sum(1 for b in z if b == 2)


def test_slot_uniformity():
    N, bins, total = 300 * 299 // 2, [0] * 16, 0
    for seed in range(40):
        for _, s in ops.region_slots(seed, [(N, 0.05, ops.STRICT, 0, 0, 0)]):
            bins[s * 16 // N] += 1
            total += 1
    chi2 = sum((b - total / 16) ** 2 / (total / 16) for b in bins)
    assert chi2 < 15 + 6 * math.sqrt(30), chi2


def test_gnm_pair_inclusion():
    hits = {}
    for seed in range(4000):
        slots = ops.gnm_slots(28, 7, seed)
        assert len(slots) == 7 == len(set(slots))
        for s in slots:
            hits[s] = hits.get(s, 0) + 1
    chi2 = sum((hits.get(s, 0) - 1000) ** 2 / 1000 for s in range(28))
    assert chi2 < 27 + 6 * math.sqrt(54), chi2


def test_gnm_dense_is_complement():
    for m in (15, 27, 28):
        slots = ops.gnm_slots(28, m, 9)
        assert len(slots) == m and slots == sorted(set(slots)) and set(slots).isdisjoint(ops.gnm_slots(28, 28 - m, 9) if m < 28 else [])


def test_below_rejects_a_third():
    N = 2 * ((1 << 64) // 3) + 1
    first_try = sum(1 for i in range(3000) if (ops.word(4, ops.TAG_GNM, 0, i) * N) & ops.M64 >= (1 << 64) % N)
    assert abs(first_try - 2000) <= 5 * math.sqrt(3000 * 2 / 9)
    assert all(0 <= ops.below(N, 4, ops.TAG_GNM, 0, i) < N for i in range(200))


def test_watts_strogatz_restated():
    assert ops.ws_edges(6, 2, 0.0, 1, undirected=False) == [(v, (v + k) % 6) for k in (1, 2) for v in range(6)]
    for flags in ((False, True), (True, False), (False, False)):
        edges = ops.ws_edges(10, 4, 0.5, 3, True, *flags)
        assert len(edges) == 40 and all(u <= v for u, v in edges)
        assert flags[0] or len(set(edges)) == 40
        assert flags[1] or all(u != v for u, v in edges)


# ------------------------------------------------------------------ fixtures from the reference's functions
def test_golden_max_edges():
    for (n, d, mu, lo), value, is_int in zip(GOLDEN["max_edges/in"].tolist(), GOLDEN["max_edges/out"].tolist(), GOLDEN["max_edges/is_int"].tolist()):
        got = gm.max_edges(n, directed=bool(d), multi_edges=bool(mu), self_loops=bool(lo))
        assert got == value and (type(got) is int) == bool(is_int)


def test_golden_likelihoods():
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or a == b                    # noqa: E731
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for i, (p, (n, m, directed)) in enumerate(zip(GOLDEN["llh/in_p"].tolist(), GOLDEN["llh/in_graph"].tolist())):
            g = Duck(n, m, bool(directed))
            if GOLDEN["llh/raised"][i]:
                for call in (lambda: gm.erdos_renyi_gnp_likelihood(p, g), lambda: gm.erdos_renyi_gnp_log_likelihood(p, g), lambda: gm.erdos_renyi_gnp_mle(g)):
                    with pytest.raises(NotImplementedError):
                        call()
                continue
            assert same(float(gm.erdos_renyi_gnp_likelihood(p, g)), float(GOLDEN["llh/likelihood"][i])), (p, n, m)
            assert same(float(gm.erdos_renyi_gnp_log_likelihood(p, g)), float(GOLDEN["llh/log_likelihood"][i])), (p, n, m)
            assert same(float(gm.erdos_renyi_gnp_mle(g)), float(GOLDEN["llh/mle"][i])), (p, n, m)


# ------------------------------------------------------------------ refusals and corner results (all before any device work)
def test_refusals():
    with pytest.raises(ValueError, match="theoretical maximum"):
        gm.erdos_renyi_gnm(5, 11)
    with pytest.raises(ValueError, match="theoretical maximum"):
        gm.erdos_renyi_gnm(5, 26, self_loops=True, directed=True)
    with pytest.raises(ValueError, match="symmetric"):
        gm.stochastic_block_model(np.array([[0.5, 0.1], [0.2, 0.5]]), [0, 1, 1])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        gm.stochastic_block_model(np.array([[0.5, 1.5], [1.5, 0.5]]), [0, 1, 1])
    with pytest.raises(ValueError, match="outside"):
        gm.stochastic_block_model(np.array([[0.5, 0.1], [0.1, 0.5]]), [0, 2, 1])
    with pytest.raises(ValueError, match="2\\^-30"):
        gm.erdos_renyi_gnp(10, 2.0 ** -31)
    with pytest.raises(ValueError, match="2\\^-30"):
        gm.stochastic_block_model(np.array([[1e-12]]), [0, 0])
    with pytest.raises(ValueError):
        gm.erdos_renyi_gnp(10, 1.5)
    with pytest.raises(ValueError, match="allow_duplicate_edges"):
        gm.watts_strogatz(4, 4, 0.1, allow_duplicate_edges=False)


def test_p_zero_and_seed():
    import torch
    for directed in (False, True):
        g = gm.erdos_renyi_gnp(7, 0.0, directed=directed, seed=12)
        assert g.n == 0 and g.m == 0 and g.mapping.num_ids() == 0 and not g.is_undirected() and g.data.edge_index.shape == (2, 0)
    for g in (gm.erdos_renyi_gnm(7, 0), gm.watts_strogatz(0, 3), gm.watts_strogatz(5, 0), gm.stochastic_block_model([[0.5]], [], seed=12)):
        assert g.n == 0 and g.m == 0 and g.mapping.num_ids() == 0 and not g.is_undirected() and not g.data.edge_index.is_cuda
    assert gm.last_seed == 12
    torch.manual_seed(77)
    gm.erdos_renyi_gnp(7, 0.0)
    first = gm.last_seed
    torch.manual_seed(77)
    gm.erdos_renyi_gnm(7, 0)
    assert gm.last_seed == first and isinstance(first, int)
