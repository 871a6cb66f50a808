"""The rolling-window kernels (csrc/pp_rolling.hip) where tests/test_gpu_rolling.py does not reach: what the DEVICE decides — an unsorted
stream, a NaN, an index outside the graph, a pair of ``max_run`` events — bit by bit against the expected status word; streams long enough
for a second grid-stride trip and windows larger than one emit workgroup; memory-resident groups (more than 2048 windows) that do not
start at window 0; the node index limits up to a window of 2^31 nodes; one emit workgroup over more windows than its LDS stage holds; and
``rolling_bounds`` alone at the ends of both time domains.  Everything is exact: indices, int32 counts and integer float32 weights."""
import numpy as np
import pytest
import torch

import cpu_ops_rolling as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip
from pathpyg_amd.algorithms import rolling_time_window as rtw
from pathpyg_amd.core.graph import Graph
from pathpyg_amd.core.index_map import IndexMap
from pathpyg_amd.data import Data, Lazy
from test_gpu_rolling import graph_of, native_only, run_native, same_graph  # noqa: F401  (native_only is a fixture)
from test_rolling_limits_host import INDEX_CASES, check_index_case, index_stream, reference_windows, windows_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, BAD_INDEX, BAD_ORDER, LONG_RUN = 0, _hip.ROLLING_BAD_INDEX, _hip.ROLLING_BAD_ORDER, _hip.ROLLING_LONG_RUN
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
M = 700                                                                # three workgroups of k_roll_keys / k_roll_count


def descents(t):
    """(by comparison: differences overflow on int64 extremes and are NaN between infinities)"""
    return int((t[:-1] > t[1:]).sum())


def base_stream(floats=False):
    ei, t = ops.random_stream(np.random.default_rng(31), M, 9, 200)
    return ei, (t.astype(np.float64) if floats else t)


def few_windows(dtype):
    """(starts, ends) of ten windows [20 i, 20 i + 25) — W <= 2048: bounds and difference array in LDS."""
    starts = np.arange(10) * 20
    return starts.astype(dtype), (starts + 25).astype(dtype)


def many_windows(dtype):
    """2500 windows [i // 10, i // 10 + 3) — W > 2048: bounds and difference array in memory."""
    starts = np.arange(2500) // 10
    return starts.astype(dtype), (starts + 3).astype(dtype)


WAYS = {
    "W <= 2048": (few_windows, None),
    "W > 2048": (many_windows, None),
    "a sub-range with w0 > 0": (few_windows, (3, 9)),
    "a memory-resident sub-range with w0 > 0": (many_windows, (100, 2400)),
}


def device_and_restated(ei, t, n, max_run=1 << 24, way="W <= 2048", restate=True):
    """``rolling_group`` -> ``rolling_bounds`` -> ``rolling_count`` on the device and, with ``restate``, on the numpy restatement:
    ``((cnt, report), (cnt, report) or None)`` as numpy arrays; ``report[-1]`` is the status word."""
    make, sub = WAYS[way]
    starts, ends = make(np.asarray(t).dtype)
    w0, w1 = sub or (0, len(starts))
    out = []
    for mod, device in ((_hip, DEV), (ops, "cpu"))[:2 if restate else 1]:
        ei_t, t_t = torch.as_tensor(np.asarray(ei)).to(device), torch.as_tensor(np.asarray(t)).to(device)
        keys, perm, flags = mod.rolling_group(ei_t, t_t, n)
        lo, hi = mod.rolling_bounds(t_t, torch.as_tensor(starts).to(device), torch.as_tensor(ends).to(device))
        cnt, report = mod.rolling_count(keys, perm, lo, hi, w0, w1, max_run, flags)
        assert report.dtype == torch.int32 and report.numel() == w1 - w0 + 2 and cnt.numel() == np.asarray(t).size
        out.append((cnt.cpu().numpy(), report.cpu().numpy()))
    return out[0], (out[1] if restate else None)


def expect_status(ei, t, n, bits, max_run=1 << 24, way="W <= 2048"):
    """The device's status word is exactly ``bits``; unless the stream is unsorted (bisection on it is implementation-defined) the counts and
    the whole report equal the restatement's too."""
    ordered = not bits & BAD_ORDER
    (cnt, report), restated = device_and_restated(ei, t, n, max_run, way, restate=ordered)
    assert int(report[-1]) == bits, (int(report[-1]), bits)
    if ordered:
        assert int(restated[1][-1]) == bits
        assert np.array_equal(report, restated[1]) and np.array_equal(cnt, restated[0])
        assert report[:-1].sum() == 0
    else:
        flags = ops.rolling_group(torch.as_tensor(np.asarray(ei)), torch.as_tensor(np.asarray(t)), n)[2]
        assert int(flags[0]) == bits & ~LONG_RUN


# ------------------------------------------------------------------ B1: order
@pytest.mark.parametrize("floats", [False, True], ids=["int64", "float64"])
@pytest.mark.parametrize("at", [0, 255, 256, 698])
def test_one_descent_is_found_wherever_it_lies(floats, at):
    """Between the first two events, across the first workgroup's edge (255, 256), behind it, and between the last two."""
    ei, t = base_stream(floats)
    t[at] = t[at + 1] + 1
    assert descents(t) == 1 and t[at] > t[at + 1]
    expect_status(ei, t, 9, BAD_ORDER)


def _signed_zeros(first, second):
    t = np.full(M, second, dtype=np.float64)
    t[:M // 2] = first
    return t


ORDERED = {
    "all 700 times equal, int64": lambda: np.full(M, 17, dtype=np.int64),
    "all 700 times equal, float64": lambda: np.full(M, 17.0),
    "-0.0 followed by +0.0": lambda: _signed_zeros(-0.0, 0.0),
    "+0.0 followed by -0.0": lambda: _signed_zeros(0.0, -0.0),
    "first time -inf": lambda: np.concatenate([[-np.inf], base_stream(True)[1][1:]]),
    "last two times +inf": lambda: np.concatenate([base_stream(True)[1][:-2], [np.inf, np.inf]]),
    "int64 from -2^63 to 2^63 - 1": lambda: np.concatenate([[I64_MIN], base_stream()[1][1:-1], [I64_MAX]]).astype(np.int64),
}


@pytest.mark.parametrize("name", list(ORDERED))
def test_streams_in_order_are_not_refused(name):
    t = ORDERED[name]()
    assert t.size == M and descents(t) == 0
    if "0.0" in name:
        assert np.signbit(t).sum() == M // 2 and (t == 0).all()
    expect_status(base_stream()[0], t, 9, OK)


@pytest.mark.parametrize("at", [0, 255, 699])
def test_one_nan_is_found_wherever_it_lies(at):
    """Also as the last event, which has no right neighbour: only ``t != t`` finds it there."""
    ei, t = base_stream(True)
    t[at] = np.nan
    expect_status(ei, t, 9, BAD_ORDER)


# ------------------------------------------------------------------ B2: index
def _with(ei, row, at, value):
    ei = ei.copy()
    ei[row, at] = value
    return ei


BAD = {
    "source n at position 0": lambda ei: (_with(ei, 0, 0, 9), 9),
    "target n at position 699": lambda ei: (_with(ei, 1, 699, 9), 9),
    "-1": lambda ei: (_with(ei, 0, 300, -1), 9),
    "2^40 with n = 9": lambda ei: (_with(ei, 1, 256, 2 ** 40), 9),
    "70000 with n = 70000 (64-bit keys)": lambda ei: (_with(ei * 7777 + 4, 0, 5, 70000), 70000),
    "65536 with n = 65536": lambda ei: (_with(ei * 8191, 1, 10, 65536), 65536),
}


@pytest.mark.parametrize("name", list(BAD))
def test_an_index_outside_the_graph_is_found(name):
    ei, t = base_stream()
    bad, n = BAD[name](ei)
    assert ((bad < 0) | (bad >= n)).sum() == 1
    good = np.where((bad < 0) | (bad >= n), 0, bad)
    expect_status(good, t, n, OK)                                      # (the same stream without the one index: accepted)
    expect_status(bad, t, n, BAD_INDEX)
    expect_status(bad, t.astype(np.float64), n, BAD_INDEX)


def test_both_16_bit_halves_full():
    """n = 65536, node 65535 on both sides: key 0xFFFFFFFF, -1 in the int32 tensor, is accepted and sorts LAST (unsigned), its three
    events are one run, and the windows that hold it come out right."""
    ei, t = base_stream()
    ei = ei * 8191                                                     # nodes 0 .. 65528
    for at in (100, 400, 699):
        ei[:, at] = 65535
    ei[:, 200], ei[:, 500] = (65535, 0), (0, 65535)
    assert _hip.rolling_key_dtype(65536) == torch.int32
    keys, perm, flags = _hip.rolling_group(torch.as_tensor(ei).to(DEV), torch.as_tensor(t).to(DEV), 65536)
    assert keys.dtype == torch.int32 and keys[-3:].tolist() == [-1, -1, -1] and perm[-3:].tolist() == [100, 400, 699]
    assert keys[-4].item() == 0xFFFF0000 - 2 ** 32 and int(flags.item()) == 0             # (65535, 0), the largest key below
    for way in WAYS:
        expect_status(ei, t, 65536, OK, way=way)
    windows = reference_windows(0, int(t[-1]), 25, 20)
    got, status = windows_of(_hip, ei, t, 65536, windows, DEV)
    assert status == 0
    for (index, weight, nodes), w in zip(got, windows):
        want = ops.brute_force(ei, t, w)
        assert np.array_equal(index, want[0]) and np.array_equal(weight, want[1]) and nodes == want[2]
    assert max(nodes for _, _, nodes in got) == 65536


# ------------------------------------------------------------------ B3: long run
def run_stream(with_2_5=True):
    """700 events on 9 nodes: pair (2, 5) exactly 130 times, pair (0, 0) exactly 40 times, each of the other 79 pairs 6 or 7 times, in a
    seeded random order.  Without (2, 5): 570 events."""
    others = [(u, v) for u in range(9) for v in range(9) if (u, v) not in ((2, 5), (0, 0))]
    pairs = [(2, 5)] * (130 if with_2_5 else 0) + [(0, 0)] * 40 + [others[i % 79] for i in range(530)]
    rng = np.random.default_rng(32)
    ei = np.array(pairs, dtype=np.int64)[rng.permutation(len(pairs))].T.copy()
    t = np.sort(rng.integers(0, 200, len(pairs))).astype(np.int64)
    return ei, t


def pair_counts(ei):
    pairs, counts = np.unique(ei.T, axis=0, return_counts=True)
    return {tuple(p): int(c) for p, c in zip(pairs.tolist(), counts)}


@pytest.mark.parametrize("way", list(WAYS))
def test_a_pair_of_max_run_events_is_flagged_and_one_event_fewer_is_not(way):
    ei, t = run_stream()
    counts = pair_counts(ei)
    assert ei.shape[1] == 700 and counts.pop((2, 5)) == 130 and counts.pop((0, 0)) == 40 and max(counts.values()) <= 30
    assert 130 > 2 * 64 and 130 % 64 != 0
    expect_status(ei, t, 9, OK, max_run=131, way=way)
    expect_status(ei, t, 9, LONG_RUN, max_run=130, way=way)
    # without (2, 5) the longest run is (0, 0)'s, key 0, at the positions 0 .. 39: the test `j >= max_run - 1` at j - (max_run - 1) == 0
    ei, t = run_stream(with_2_5=False)
    assert ei.shape[1] == 570 and max(pair_counts(ei).values()) == 40 == pair_counts(ei)[(0, 0)]
    keys = _hip.rolling_group(torch.as_tensor(ei).to(DEV), torch.as_tensor(t).to(DEV), 9)[0]
    assert keys[:41].tolist() == [0] * 40 + [1]
    expect_status(ei, t, 9, OK, max_run=41, way=way)
    expect_status(ei, t, 9, LONG_RUN, max_run=40, way=way)
    expect_status(ei, t, 9, LONG_RUN, max_run=1, way=way)              # every event is a run of one
    expect_status(ei[:, :1], t[:1], 9, LONG_RUN, max_run=1, way=way)
    expect_status(ei[:, :1], t[:1], 9, OK, max_run=2, way=way)


def test_descent_bad_index_and_long_run_together():
    ei, t = run_stream()
    t[500] = t[501] + 1
    others = [i for i in range(700) if ei[:, i].tolist() != [2, 5]]
    ei[0, others[3]], ei[1, others[-2]] = -1, 9
    assert ((ei < 0) | (ei >= 9)).sum() == 2 and pair_counts(ei)[(2, 5)] == 130 and descents(t) == 1
    for way in WAYS:
        expect_status(ei, t, 9, BAD_INDEX | BAD_ORDER | LONG_RUN, max_run=130, way=way)
        assert BAD_INDEX | BAD_ORDER | LONG_RUN == 7


@pytest.mark.parametrize("held", [0, 2, 3])
def test_without_events_the_report_is_zeros_and_the_flags(held):
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    bounds = torch.zeros(3, dtype=torch.int32, device=DEV)
    flags = torch.tensor([held], dtype=torch.int32, device=DEV)
    cnt, report = _hip.rolling_count(empty, empty, bounds, bounds, 0, 3, 5, flags)
    assert cnt.numel() == 0 and report.tolist() == [0, 0, 0, 0, held]
    cnt, report = _hip.rolling_count(empty, empty, bounds, bounds, 1, 3, 5, flags)
    assert report.tolist() == [0, 0, 0, held]


# ------------------------------------------------------------------ B4: through the public functions
@pytest.mark.parametrize("case", ["unsorted", "nan", "index", "long run"])
def test_what_the_device_finds_sends_the_public_functions_to_the_per_window_call(native_only, monkeypatch, case):
    reads, _ = native_only
    ei, t = run_stream() if case == "long run" else base_stream(floats=case == "nan")
    g = graph_of(ei, t, 9)
    if case == "unsorted":
        g.data.time[300] = g.data.time[301] + 1
    elif case == "nan":
        g.data.time[255] = float("nan")
    elif case == "index":
        assert ei.max() == 8
        g.data.num_nodes = 8
    else:
        monkeypatch.setattr(rtw, "MAX_RUN", 130)
    fills = []
    fill = _hip.rolling_fill
    monkeypatch.setattr(_hip, "rolling_fill", lambda *a, **k: fills.append(1) or fill(*a, **k))
    size, step = (25.0, 20.0) if case == "nan" else (25, 20)
    assert rtw.eligible(g, size, step)
    assert pp.algorithms.rolling_static_graphs(g, size, step) is None and reads == [1] and fills == []
    windows = reference_windows(g.start_time, g.end_time, size, step)
    assert len(windows) >= 9
    items = list(pp.algorithms.RollingTimeWindow(g, size, step, return_window=True))
    assert [w for _, w in items] == windows and reads == [1, 1] and fills == []              # decided once, by one read-back
    for got, w in items:
        same_graph(got, g.to_static_graph(weighted=True, time_window=w))


def test_one_event_below_max_run_stays_native(native_only, monkeypatch):
    ei, t = run_stream()
    monkeypatch.setattr(rtw, "MAX_RUN", 131)
    items = run_native(graph_of(ei, t, 9), 25, 20, native_only)
    assert max(s.data.edge_weight.max().item() for s, _ in items) > 10


# ------------------------------------------------------------------ C1: a second grid-stride trip, windows above one emit workgroup
LONG_M = 2048 * 256 + 300


@pytest.fixture(scope="module")
def long_stream():
    ei, t = ops.random_stream(np.random.default_rng(33), LONG_M, 300, 400)
    t[0], t[-1] = 0, 399                                               # (still sorted)
    return ei, t


def test_long_stream_every_window_equals_the_per_window_call(native_only, long_stream):
    """524 588 events: the grid of 2048 workgroups of 256 threads takes a second trip in k_roll_keys, k_roll_count (whose LDS difference
    array then accumulates over two trips) and k_roll_fill; four windows of about 131 000 events and tens of thousands of distinct pairs
    each: many k_roll_emit workgroups meet in one window's node count."""
    ei, t = long_stream
    m = ei.shape[1]
    assert m > 2048 * 256 and m == LONG_M
    g = graph_of(ei, t, 300)
    items = run_native(g, 100, 100, native_only, expect_windows=4)
    assert all(s.data.edge_index.size(1) > 10_000 > 1024 for s, _ in items)
    assert sum(s.data.edge_weight.sum().item() for s, _ in items) == m
    for i in (0, 3):
        s, w = items[i]
        want_index, want_weight, want_nodes = ops.brute_force(ei, t, w)
        assert np.array_equal(s.data.edge_index.cpu().numpy(), want_index) and np.array_equal(s.data.edge_weight.cpu().numpy(), want_weight)
        assert s.n == want_nodes


@pytest.mark.parametrize("case", ["descent", "index"])
def test_long_stream_refusals_in_the_second_trip(long_stream, case):
    """The last two events are reached only in the second trip of k_roll_keys' loop (i >= 2048 * 256)."""
    ei, t = long_stream
    m = ei.shape[1]
    assert m - 2 >= 2048 * 256
    ei_t, t_t = torch.as_tensor(ei).to(DEV), torch.as_tensor(t).to(DEV)
    if case == "descent":
        t_t[m - 2] = t_t[m - 1] + 1
    else:
        ei_t[1, m - 1] = 300
    keys, perm, flags = _hip.rolling_group(ei_t, t_t, 300)
    starts = torch.tensor([0, 100, 200, 300], device=DEV)
    lo, hi = _hip.rolling_bounds(t_t, starts, starts + 100)
    _, report = _hip.rolling_count(keys, perm, lo, hi, 0, 4, 1 << 24, flags)
    assert report[-1].item() == (BAD_ORDER if case == "descent" else BAD_INDEX)


# ------------------------------------------------------------------ C2: memory-resident groups that do not start at window 0
def test_two_groups_above_the_lds_tables(native_only, monkeypatch):
    """About 4700 sparse windows cut into two groups of more than 2048 windows each: both take the memory-resident form of k_roll_count and
    k_roll_fill, the second one with w0 > 0 (bounds read at their global index, difference array at ``a - w0``)."""
    reads, arm = native_only
    ei, t = ops.random_stream(np.random.default_rng(34), 3000, 20, 9400)
    t[0], t[-1] = 0, 9399
    windows = reference_windows(0, 9399, 5, 2)
    want = [ops.brute_force(ei, t, w) for w in windows]
    counts = [x[0].shape[1] for x in want]
    budget = int(sum(counts) * 0.52)
    monkeypatch.setattr(rtw, "BATCH_EDGES", budget)
    groups = rtw.window_groups(counts, budget)
    assert len(windows) == 4700 and len(groups) == 2
    assert all(w1 - w0 > 2048 for w0, w1 in groups) and groups[1][0] > 0 and groups[0][1] == groups[1][0] and groups[1][1] == 4700
    g = graph_of(ei, t, 20)
    fills = []
    fill = _hip.rolling_fill
    monkeypatch.setattr(_hip, "rolling_fill", lambda *a, **k: fills.append((a[5], a[6], a[8])) or fill(*a, **k))
    arm()
    batch = pp.algorithms.rolling_static_graphs(g, 5, 2)
    assert batch.windows == windows and reads == [1]
    assert [(a, b) for a, b, _ in fills] == groups and [total for _, _, total in fills] == [sum(counts[a:b]) for a, b in groups]
    index, weight, ptr = batch.edge_index.cpu().numpy(), batch.edge_weight.cpu().numpy(), batch.win_ptr_host
    assert np.diff(ptr).tolist() == counts
    for i, (want_index, want_weight, want_nodes) in enumerate(want):
        assert np.array_equal(index[:, ptr[i]:ptr[i + 1]], want_index) and np.array_equal(weight[ptr[i]:ptr[i + 1]], want_weight), i
        assert batch.num_nodes[i] == want_nodes, i


# ------------------------------------------------------------------ C3: index limits
@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_kernels_at_the_node_index_limits(name):
    """Direct calls (num_nodes is a plain int there, nothing is O(n)): against brute force; the window whose one edge holds node 2^31 - 1
    has 2^31 nodes."""
    check_index_case(_hip, name, DEV)


def test_key_width_flips_at_65537_nodes():
    assert _hip.rolling_key_dtype(65536) == torch.int32 and _hip.rolling_key_dtype(65537) == torch.int64
    for n, top in (INDEX_CASES["n = 65536: both 16-bit halves full"], INDEX_CASES["n = 65537: the first 64-bit keys"]):
        ei, t = index_stream(n, top)
        keys = _hip.rolling_group(torch.as_tensor(ei).to(DEV), torch.as_tensor(t).to(DEV), n)[0]
        assert keys.dtype == (torch.int32 if n == 65536 else torch.int64)
        assert keys[-1].item() == (-1 if n == 65536 else (65536 << 17) | 65536)


class DeviceStream:
    """What RollingTimeWindow reads of a TemporalGraph, over device tensors; ``to_static_graph`` is the brute force on the host, moved to
    the device, with the node_sequence left unmade."""

    def __init__(self, edge_index, time, num_nodes):
        self.host = (np.asarray(edge_index), np.asarray(time))
        self.data = Data(edge_index=torch.as_tensor(self.host[0]).to(DEV), time=torch.as_tensor(self.host[1]).to(DEV), num_nodes=num_nodes)
        self.mapping = IndexMap()
        self.calls = []

    @property
    def start_time(self):
        return self.data.time[0].item()

    @property
    def end_time(self):
        return self.data.time[-1].item()

    def to_static_graph(self, weighted=False, time_window=None):
        self.calls.append((weighted, time_window))
        index, weight, n = ops.brute_force(*self.host, time_window)
        data = Data(edge_index=torch.from_numpy(index).to(DEV), edge_weight=torch.from_numpy(weight).to(DEV), num_nodes=n,
                    node_sequence=Lazy(lambda: torch.arange(n, device=DEV).reshape(-1, 1), (n, 1)))
        return Graph(data, self.mapping, _row_sorted=True)


@pytest.mark.parametrize("size,step", [(3, 3), (5, 2)])
def test_a_graph_of_two_to_the_31_nodes_through_the_iterator(size, step):
    """num_nodes = 2^31 with node 2^31 - 1 present.  ``TemporalGraph.to_static_graph`` makes a node_sequence of num_nodes rows for every
    window — 16 GiB each here — so the public-level check goes through a stand-in with the attributes RollingTimeWindow reads, over device
    tensors, whose per-window call is the brute force and does not raise: every item must equal it, with 2^31 nodes."""
    n, top = INDEX_CASES["n = 2^31: a window of 2^31 nodes"]
    ei, t = index_stream(n, top)
    stream = DeviceStream(ei, t, n)
    assert rtw.eligible(stream, size, step)
    items = list(pp.algorithms.RollingTimeWindow(stream, size, step, return_window=True))
    assert stream.calls == [] and [w for _, w in items] == reference_windows(0, 10, size, step)
    for got, w in items:
        want = stream.to_static_graph(weighted=True, time_window=w)
        assert torch.equal(got.data.edge_index, want.data.edge_index) and torch.equal(got.data.edge_weight, want.data.edge_weight)
        assert got.n == got.data.num_nodes == want.n == 2 ** 31 and type(got.data.num_nodes) is int
        assert got.data.peek("node_sequence").shape == (2 ** 31, 1) and got.mapping is stream.mapping


# ------------------------------------------------------------------ C4: k_roll_emit beyond its LDS span
def test_one_emit_workgroup_over_more_windows_than_its_stage_holds(native_only):
    """320 windows of 1 to 8 edges: the 1024 edges of the first k_roll_emit workgroup span more than 200 windows, its LDS stage of the node
    maxima holds 64 — the others go to memory directly.  Window w's largest node, 10 + w % 50, is in one edge only."""
    reads, arm = native_only
    events = []
    for w in range(320):
        events.append((10 + w % 50, w % 5, w))
        events += [(i, (i + w) % 9, w) for i in range((w * 7) % 8)]
    ei = np.array([[u for u, _, _ in events], [v for _, v, _ in events]], dtype=np.int64)
    t = np.array([x for _, _, x in events], dtype=np.int64)
    windows = reference_windows(0, 319, 1, 1)
    want = [ops.brute_force(ei, t, w) for w in windows]
    largest = max(x[0].shape[1] for x in want)
    assert len(windows) == 320 >= 300 and largest <= 8 and 64 * largest < 1024 and sum(x[0].shape[1] for x in want) > 1024
    assert all(x[2] == 10 + w % 50 + 1 and (x[0] == x[2] - 1).sum() == 1 for w, x in enumerate(want))
    g = graph_of(ei, t, 60)
    arm()
    batch = pp.algorithms.rolling_static_graphs(g, 1, 1)
    assert batch.windows == windows and reads == [1]
    assert batch.num_nodes == [x[2] for x in want]
    index, weight, ptr = batch.edge_index.cpu().numpy(), batch.edge_weight.cpu().numpy(), batch.win_ptr_host
    for i, (want_index, want_weight, _) in enumerate(want):
        assert np.array_equal(index[:, ptr[i]:ptr[i + 1]], want_index) and np.array_equal(weight[ptr[i]:ptr[i + 1]], want_weight), i


# ------------------------------------------------------------------ C5: rolling_bounds alone
def _bounds_case(name):
    rng = np.random.default_rng(35)
    if name == "int64 ends":
        t = np.sort(rng.integers(-50, 50, M)).astype(np.int64)
        t[:2], t[-2:] = I64_MIN, I64_MAX
        cuts = np.sort(rng.integers(-60, 60, 257)).astype(np.int64)
        starts, ends = cuts.copy(), cuts + 7
        starts[:3], ends[:2], starts[-1], ends[-3:] = I64_MIN, I64_MIN, I64_MAX, I64_MAX
    else:
        t = np.sort(rng.integers(-50, 50, M)).astype(np.float64) / 4
        t[:2], t[-2:] = -np.inf, np.inf
        cuts = np.sort(rng.integers(-60, 60, 257)).astype(np.float64) / 4
        starts, ends = cuts.copy(), cuts + 1.75
        starts[:3], ends[:2], starts[-1], ends[-3:] = -np.inf, -np.inf, np.inf, np.inf
    return t, starts, ends


@pytest.mark.parametrize("name", ["int64 ends", "float64 infinities"])
def test_rolling_bounds_at_the_ends_of_the_time_domain(name):
    """257 windows: the second workgroup has one live thread.  Starts and ends at the smallest and largest value of the dtype — -2^63 and
    2^63 - 1, -inf and +inf — over a stream that begins and ends with two such events."""
    t, starts, ends = _bounds_case(name)
    assert starts.size == 257 and descents(t) == 0 and descents(starts) == 0 and descents(ends) == 0
    lo, hi = _hip.rolling_bounds(torch.as_tensor(t).to(DEV), torch.as_tensor(starts).to(DEV), torch.as_tensor(ends).to(DEV))
    assert lo.dtype == hi.dtype == torch.int32
    want_lo, want_hi = np.searchsorted(t, starts, side="left"), np.searchsorted(t, ends, side="left")
    assert np.array_equal(lo.cpu().numpy(), want_lo) and np.array_equal(hi.cpu().numpy(), want_hi)
    assert want_lo[0] == 0 and want_hi[0] == 0 and want_lo[-1] == M - 2 and want_hi[-1] == M - 2 and 2 < want_lo[128] < M - 2
