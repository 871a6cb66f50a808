"""RollingTimeWindow on the device (csrc/pp_rolling.hip): every item equals ``TemporalGraph.to_static_graph(weighted=True, time_window=w)`` of
the same graph bit for bit — edge_index, edge_weight, num_nodes, the window — at the smallest shapes at which the kernels can go wrong; on
the native path the per-window call is never made and the window counts are read back once per iterator; the fallbacks still equal the
per-window call."""
import numpy as np
import pytest
import torch

import cpu_ops_rolling as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip
from pathpyg_amd.algorithms import rolling_time_window as rtw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

REFERENCE_EXAMPLE = [("a", "b", 1), ("b", "c", 5), ("c", "d", 9), ("c", "e", 9), ("c", "f", 11), ("f", "a", 13), ("a", "g", 18), ("b", "f", 21),
                     ("a", "g", 26), ("c", "f", 27), ("h", "f", 27), ("g", "h", 28), ("a", "c", 30), ("a", "b", 31), ("c", "h", 32), ("f", "h", 33),
                     ("b", "i", 42), ("i", "b", 42), ("c", "i", 47), ("h", "i", 50)]


def graph_of(ei, t, n, device=DEV):
    return pp.TemporalGraph(pp.Data(edge_index=torch.as_tensor(np.asarray(ei)).to(device), time=torch.as_tensor(np.asarray(t)).to(device), num_nodes=n))


def per_window(g, windows, weighted=True):
    return [g.to_static_graph(weighted=weighted, time_window=w) for w in windows]


def same_graph(got, want, weighted=True):
    assert got.data.edge_index.dtype == want.data.edge_index.dtype == torch.int64
    assert torch.equal(got.data.edge_index, want.data.edge_index)
    if weighted:
        assert got.data.edge_weight.dtype == want.data.edge_weight.dtype == torch.float32
        assert torch.equal(got.data.edge_weight, want.data.edge_weight)
    else:
        assert "edge_weight" not in got.data
    assert got.n == want.n and got.data.num_nodes == want.data.num_nodes and got.mapping is want.mapping
    assert torch.equal(got.data.node_sequence, want.data.node_sequence) and got.data.edge_index.device == want.data.edge_index.device


@pytest.fixture
def native_only(monkeypatch):
    """After ``arm()`` the per-window call raises; ``reads`` counts the count read-backs."""
    reads = []
    read = rtw._read_report
    monkeypatch.setattr(rtw, "_read_report", lambda report: reads.append(1) or read(report))

    def arm():
        def refuse(self, *a, **k):
            raise AssertionError("to_static_graph was called on the native path")
        monkeypatch.setattr(pp.TemporalGraph, "to_static_graph", refuse)
    reads_and_arm = (reads, arm)
    return reads_and_arm


def run_native(g, size, step, native_only, expect_windows=None):
    reads, arm = native_only
    windows, after = rtw.schedule(g.start_time, g.end_time, size, step)
    if expect_windows is not None:
        assert len(windows) == expect_windows
    want = per_window(g, windows)
    arm()
    r = pp.algorithms.RollingTimeWindow(g, size, step, return_window=True)
    items = list(r)
    assert [w for _, w in items] == windows and r.current_time == after and type(r.current_time) is type(after)
    for (got, _), ref in zip(items, want):
        same_graph(got, ref)
    assert reads == [1]
    return items


def test_reference_docstring_example(native_only):
    g = pp.TemporalGraph.from_edge_list(REFERENCE_EXAMPLE, device=DEV)
    items = run_native(g, 10, 10, native_only)
    assert [w for _, w in items] == [(1, 11), (11, 21), (21, 31), (31, 41), (41, 51)]
    assert [s.data.edge_index.size(1) for s, _ in items] == [4, 3, 6, 3, 4]
    assert [s.n for s, _ in items] == [5, 7, 8, 8, 9]
    assert items[0][0].data.edge_index.tolist() == [[0, 1, 2, 2], [1, 2, 3, 4]] and items[0][0].data.edge_weight.tolist() == [1.0] * 4
    assert items[0][0].mapping is g.mapping


def _stream(seed, m, n, span, floats=False):
    return ops.random_stream(np.random.default_rng(seed), m, n, span, floats)


def _one_pair_of_200():
    """Pair (2, 5) at every third time unit, 200 times, inside 300 other events: a run longer than a wave, crossing many windows."""
    rng = np.random.default_rng(6)
    ei = np.concatenate([np.tile([[2], [5]], 200), rng.integers(0, 8, (2, 300))], axis=1)
    t = np.concatenate([np.arange(200) * 3, rng.integers(0, 600, 300)])
    order = np.argsort(t, kind="stable")
    return ei[:, order], t[order], 8, 40, 15, None


def _w300():
    ei, t = _stream(8, 2000, 30, 1500)
    t[0], t[-1] = 0, 1499                                   # (still sorted) 300 starts 0, 5, ..., 1495: the window sort takes two digit passes
    return ei, t, 30, 9, 5, 300


def _two_bursts():
    t = np.sort(np.concatenate([np.arange(200) % 20, 100 + np.arange(200) % 30]))
    return _stream(5, 400, 7, 1)[0], t, 7, 8, 8, None


# name: () -> (edge_index, time, n, window_size, step_size, number of windows or None)
SHAPES = {
    "one event": lambda: ([[3], [1]], [7], 5, 4, 2, 1),
    "one window": lambda: (*_stream(1, 300, 9, 50), 9, 1000, 1000, 1),
    "all events at one timestamp": lambda: (_stream(2, 500, 6, 1)[0], np.full(500, 17), 6, 3, 1, 1),
    "ties straddling a window end": lambda: ([[0, 0, 0, 1, 0, 0, 1], [1, 1, 1, 0, 1, 1, 0]], [0, 4, 4, 4, 5, 5, 9], 2, 5, 5, 2),
    "step above the size": lambda: (*_stream(3, 700, 12, 90), 12, 3, 10, None),
    "step below the size": lambda: (*_stream(4, 700, 12, 60), 12, 24, 2, None),
    "empty windows in the middle": _two_bursts,
    "one pair of 200 events across many windows": _one_pair_of_200,
    "m = 5000: sort tiles and blocks with a tail": lambda: (*_stream(7, 5000, 300, 400), 300, 25, 25, None),
    "W = 300 on 2000 events": _w300,
    "float64 times, fractional step": lambda: (*_stream(9, 900, 15, 240, floats=True), 15, 2.75, 0.7, None),
    "64-bit keys": lambda: (_stream(10, 800, 70000, 1)[0], _stream(10, 800, 4, 64)[1], 70000, 7, 3, None),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_window_equals_the_per_window_call(native_only, name):
    ei, t, n, size, step, expect = SHAPES[name]()
    g = graph_of(ei, t, n)
    assert g.data.time.dtype == (torch.float64 if isinstance(step, float) else torch.int64)
    items = run_native(g, size, step, native_only, expect)
    counts = [s.data.edge_index.size(1) for s, _ in items]
    if name == "step above the size":
        assert sum(s.data.edge_weight.sum().item() for s, _ in items) < g.data.time.numel()          # events in no window
    if name == "step below the size":
        assert sum(s.data.edge_weight.sum().item() for s, _ in items) > 5 * g.data.time.numel()      # an event in many windows
    if name == "empty windows in the middle":
        assert 0 in counts[1:-1] and counts[0] > 0 and counts[-1] > 0
    if name == "one pair of 200 events across many windows":
        assert max(s.data.edge_weight.max().item() for s, _ in items) >= 14 and len(items) > 30
    if name == "64-bit keys":
        assert _hip.rolling_key_dtype(n) == torch.int64 and max(s.n for s, _ in items) > 65536


def test_more_windows_than_the_lds_tables_hold(native_only):
    """W = 2500 > 2048: bounds and difference array in memory instead of LDS.  Every window against the brute force on the host, every 50th
    against the per-window call."""
    reads, arm = native_only
    ei, t = _stream(11, 3000, 20, 5000)
    g = graph_of(ei, t, 20)
    windows, _ = rtw.schedule(g.start_time, g.end_time, 5, 2)
    assert len(windows) > 2048 + 256
    sample = {i: g.to_static_graph(weighted=True, time_window=windows[i]) for i in range(0, len(windows), 50)}
    arm()
    batch = pp.algorithms.rolling_static_graphs(g, 5, 2)
    assert batch.windows == windows and reads == [1]
    index, weight, ptr = batch.edge_index.cpu().numpy(), batch.edge_weight.cpu().numpy(), batch.win_ptr.cpu().numpy()
    assert ptr.tolist() == list(batch.win_ptr_host)
    for i, w in enumerate(windows):
        want_index, want_weight, want_n = ops.brute_force(ei, t, w)
        assert np.array_equal(index[:, ptr[i]:ptr[i + 1]], want_index) and np.array_equal(weight[ptr[i]:ptr[i + 1]], want_weight)
        assert batch.num_nodes[i] == want_n
    for i, ref in sample.items():
        same_graph(batch.graph(i), ref)


def test_several_groups_and_a_window_above_the_budget(native_only, monkeypatch):
    ei, t = _stream(12, 1500, 10, 200)
    g = graph_of(ei, t, 10)
    monkeypatch.setattr(rtw, "BATCH_EDGES", 150)
    fills = []
    fill = _hip.rolling_fill
    monkeypatch.setattr(_hip, "rolling_fill", lambda *a, **k: fills.append((a[5], a[6], a[8])) or fill(*a, **k))
    items = run_native(g, 8, 6, native_only)              # a window of 8 time units holds about 45 of the 100 pairs
    counts = [s.data.edge_index.size(1) for s, _ in items]
    assert len(fills) >= 3 and [(a, b) for a, b, _ in fills] == rtw.window_groups(counts, 150)
    assert all(total == sum(counts[a:b]) <= 150 for a, b, total in fills) and any(b - a > 1 for a, b, _ in fills)
    monkeypatch.setattr(rtw, "BATCH_EDGES", 30)           # now most windows are above the budget, each a group of its own
    del fills[:]
    batch = pp.algorithms.rolling_static_graphs(g, 8, 6)
    assert [(a, b) for a, b, _ in fills] == rtw.window_groups(counts, 30)
    assert sum(1 for a, b, total in fills if total > 30 and b == a + 1) >= 10 and all(total <= 30 or b == a + 1 for a, b, total in fills)
    assert np.diff(batch.win_ptr_host).tolist() == counts
    for i, (s, _) in enumerate(items):
        same_graph(batch.graph(i), s)


def test_graph_views_launch_nothing_and_read_nothing_back(monkeypatch):
    ei, t = _stream(13, 400, 9, 80)
    g = graph_of(ei, t, 9)
    batch = pp.algorithms.rolling_static_graphs(g, 10, 5)
    for name in ("minmax", "is_sorted", "stable_argsort", "coalesce"):
        monkeypatch.setattr(pp.core.graph._dispatch, name, lambda *a, **k: pytest.fail("a kernel behind RollingWindows.graph"))
    monkeypatch.setattr(torch, "arange", lambda *a, **k: pytest.fail("torch.arange behind RollingWindows.graph"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a read-back behind RollingWindows.graph"))
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: pytest.fail("a read-back behind RollingWindows.graph"))
    graphs = [batch.graph(i) for i in range(len(batch))]
    assert [s.n for s in graphs] == batch.num_nodes and [s.data.num_edges for s in graphs] == np.diff(batch.win_ptr_host).tolist()
    assert all(isinstance(s.data.peek("node_sequence"), pp.data.Lazy) and s.order == 1 for s in graphs)      # made when somebody reads it
    assert graphs[0].data.edge_index.data_ptr() == batch.edge_index.data_ptr()
    assert graphs[0].data.edge_weight.data_ptr() == batch.edge_weight.data_ptr()


@pytest.mark.parametrize("case", ["unweighted", "float step on integer times", "switched off", "host graph"])
def test_fallbacks_equal_the_per_window_call(monkeypatch, case):
    ei, t = _stream(14, 300, 8, 60)
    g = graph_of(ei, t, 8, device="cpu" if case == "host graph" else DEV)
    size, step, weighted = (10, 2.5, True) if case.startswith("float") else (10, 7, case != "unweighted")
    windows, after = [], g.start_time
    while after <= g.end_time:
        windows.append((after, after + size))
        after += step
    want = per_window(g, windows, weighted)
    for name in ("rolling_group", "rolling_bounds", "rolling_count", "rolling_fill"):
        monkeypatch.setattr(_hip, name, lambda *a, **k: pytest.fail("a rolling kernel ran on a fallback path"))
    if case == "switched off":
        monkeypatch.setattr(rtw, "NATIVE", False)
    r = pp.algorithms.RollingTimeWindow(g, size, step, return_window=True, weighted=weighted)
    items = list(r)
    assert [w for _, w in items] == windows and r.current_time == after
    for (got, _), ref in zip(items, want):
        same_graph(got, ref, weighted)
    if case == "unweighted":
        assert sum(s.data.edge_index.size(1) for s, _ in items) > 300                 # multi-edges kept, in event order
