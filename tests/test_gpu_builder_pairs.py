"""k_db2_mid works on two middle nodes per wave (csrc/pp_debruijn.hip, db2_mid_pair): nodes 2k and 2k+1 side by side in the two halves of
the wave where both have at most 32 in- and 32 out-events and take the fast paths, one after the other otherwise.  The streams here are
built from explicit (src, dst, t) lists so that a pair has exactly the intended in- and out-lists: every test node's events go to / come
from filler nodes that are used once, so in-events come from distinct sources and successor runs are single events unless a case says
otherwise.  Every case builds with the fused builder and with the generic kernels (the reference: not the code under test) and requires
every plan array, dst_order, the bipartite arrays, indeg and the sizes to be equal bit for bit; the sizes of the boundary sets are also
held to the CPU oracle, which guards against both GPU paths being wrong together."""
import numpy as np
import pytest
import torch

from test_gpu_builder import _build, _compare, _stream

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 31, 32, 33, 64, 65)          # around the half-wave (paired / one after the other) and the wave (hub) limits
PARTNER = (20, 20)
SPAN = 3000


class _Stream:
    """Events of test nodes 0 .. k-1 (node i with specs[i] = (in-events, out-events)); filler nodes are numbered from k on, each used once."""

    def __init__(self, specs, seed, span=SPAN):
        self.rng = np.random.default_rng(seed)
        self.span = span
        self.k = len(specs)
        self.next = self.k
        self.ev = []
        for b, (ni, no) in enumerate(specs):
            for _ in range(ni):
                self.add(self.filler(), b)
            for _ in range(no):
                self.add(b, self.filler())

    def filler(self):
        self.next += 1
        return self.next - 1

    def add(self, src, dst, t=None):
        self.ev.append((src, dst, int(self.rng.integers(0, self.span)) if t is None else t))

    def tensors(self, time_dtype=torch.int64, n=None):
        ev = sorted(self.ev, key=lambda e: e[2])                   # (stable: ties keep their order)
        ei = torch.tensor([[e[0] for e in ev], [e[1] for e in ev]], dtype=torch.int64).reshape(2, -1)
        t = torch.tensor([e[2] for e in ev], dtype=torch.int64)
        if time_dtype == torch.float64:
            t = t.to(torch.float64) * 0.25                         # (quarters: timestamp ties stay ties)
        return ei, t, (self.next if n is None else n)


def _boundary_specs(position, hub):
    """Every (ni, no) of SIZES x SIZES with (hub) or without a list of 65, beside the partner, the node under test first or second."""
    specs = []
    for ni in SIZES:
        for no in SIZES:
            if (ni > 64 or no > 64) != hub:
                continue
            specs += [(ni, no), PARTNER] if position == 0 else [PARTNER, (ni, no)]
    return specs


VARIANTS = {
    # time dtype, delta, fractional weights
    "plain": (torch.int64, 700, False),
    "float64-times": (torch.float64, 175.25, False),
    "fractional-weights": (torch.int64, 700, True),
    "float-delta": (torch.int64, 700.5, False),
    "delta-zero": (torch.int64, 0, False),
    "delta-everything": (torch.int64, 10 ** 9, False),
}


def _weights(m, seed):
    return torch.from_numpy(np.random.default_rng(seed).random(m).astype(np.float32) + 0.25)


def _oracle_sizes(ei, t, n, delta):
    from oracle import model as om
    from oracle.lift import temporal_lift_sorted
    sei, st, _ = om.stable_time_sort(ei, t)
    want = om.layers_from_temporal(sei, st, n, delta=delta, max_order=2)
    return {"E2": int(temporal_lift_sorted(sei, st, delta, n).size(1)), "U2": want[2]["num_nodes"], "A1": want[1]["edge_index"].size(1),
            "A2": want[2]["edge_index"].size(1)}


def _check(ei, t, n, delta, w=None, hubs=False, oracle=False):
    fused, generic = _build(ei, t, n, delta, w, True), _build(ei, t, n, delta, w, False)
    _compare(fused, generic, hubs=hubs, float_rtol=1e-5 if (hubs and w is not None) else None)
    if oracle:
        want = _oracle_sizes(ei, t, n, delta)
        for k, v in want.items():
            assert fused.sizes[k] == v, f"sizes[{k}]: {fused.sizes[k]} != oracle's {v}"


@pytest.mark.parametrize("n,events", [
    (1, [(0, 0, 1), (0, 0, 2), (0, 0, 2), (0, 0, 5)]),
    (2, [(0, 1, 1), (1, 0, 2), (0, 1, 3), (1, 1, 3), (1, 0, 4), (0, 0, 6)]),
    (3, [(0, 1, 1), (1, 2, 2), (2, 0, 3), (0, 2, 3), (2, 1, 4), (1, 2, 5), (2, 2, 6), (2, 0, 7)]),
], ids=["n1", "n2", "n3"])
def test_tiny_node_sets(n, events):
    ei = torch.tensor([[e[0] for e in events], [e[1] for e in events]], dtype=torch.int64)
    t = torch.tensor([e[2] for e in events], dtype=torch.int64)
    _check(ei, t, n, 2, oracle=n > 1)                             # (the oracle's aggregate squeezes a one-node sequence to a scalar: no n = 1 there)


def test_odd_node_count_whose_last_node_has_events():
    ei, t = _stream(61, 3000, 151, 2000)
    ei[0, :15] = 150
    ei[1, 15:30] = 150
    _check(ei, t, 151, 150, oracle=True)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("hub", [False, True], ids=["fits", "hub"])
@pytest.mark.parametrize("position", [0, 1], ids=["first", "second"])
def test_list_lengths_at_the_half_wave_and_wave_limits(position, hub, variant):
    tdt, delta, weighted = VARIANTS[variant]
    ei, t, n = _Stream(_boundary_specs(position, hub), seed=70 + position).tensors(tdt)
    w = _weights(ei.size(1), 71) if weighted else None
    _check(ei, t, n, delta, w, hubs=hub, oracle=True)


def test_divergent_trip_counts_within_a_pair():
    specs = [(1, 32), (32, 1), (32, 1), (1, 32), (0, 0), (32, 32), (32, 32), (0, 0), (32, 0), (0, 32), (1, 1), (32, 32)]
    ei, t, n = _Stream(specs, seed=72).tensors()
    _check(ei, t, n, 900, oracle=True)
    _check(ei, t, n, 900, _weights(ei.size(1), 73))


def _mixed_routes():
    """Per kind and position: a pair of a node that cannot take the fast path and a simple partner."""
    kinds = ("same-source", "again", "self-loop", "two-self-loops")
    s = _Stream([PARTNER] * (2 * 2 * len(kinds)), seed=74)         # (every node starts as a simple (20, 20) node; one of each pair gets extras)
    for i, kind in enumerate(kinds):
        for position in (0, 1):
            b = 2 * (2 * i + position) + position
            if kind == "same-source":                              # two in-events from one source: an in-run of two events
                a = s.filler()
                s.add(a, b, 1000)
                s.add(a, b, 1400)
            elif kind == "again":                                  # one in-event reaches a two-event successor run twice within delta
                c = s.filler()
                s.add(s.filler(), b, 1500)
                s.add(b, c, 1510)
                s.add(b, c, 1520)
            elif kind == "self-loop":                              # an event (b, b): in-event from the node itself, out-event to itself
                s.add(b, b, 1200)
            else:                                                  # (b, b) -> (b, b): a self loop of the order-2 graph as well
                s.add(b, b, 1200)
                s.add(b, b, 1700)
    return s.tensors()


@pytest.mark.parametrize("weighted", [False, True], ids=["unit-weights", "fractional-weights"])
def test_mixed_routes_within_a_pair(weighted):
    ei, t, n = _mixed_routes()
    _check(ei, t, n, 700, _weights(ei.size(1), 75) if weighted else None, oracle=not weighted)


@pytest.mark.parametrize("n,m", [(300, 6000), (200, 6000)], ids=["mean20", "mean30"])
def test_headline_shaped_random_streams(n, m):
    ei, t = _stream(76, m, n, 100000)
    _check(ei, t, n, 30000)
    _check(ei, t, n, 30000, _weights(m, 77))
