"""Host side of RollingTimeWindow (algorithms/rolling_time_window.py): the numpy restatement of the kernels (tests/cpu_ops_rolling.py) run
through the package's own planning, grouping and iteration code reproduces brute force on seeded random streams; the window schedule is the
reference's (repeated addition); eligibility, the greedy groups under BATCH_EDGES, the fallbacks, and the header.  No GPU."""
import re

import numpy as np
import pytest
import torch

import cpu_ops_rolling as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip, _lib
from pathpyg_amd.algorithms import rolling_time_window as rtw
from pathpyg_amd.core.graph import Graph
from pathpyg_amd.core.index_map import IndexMap
from pathpyg_amd.data import Data

NEW_FUNCTIONS = ("pp_rolling_key_bytes", "pp_rolling_group_ws_bytes", "pp_rolling_group", "pp_rolling_bounds", "pp_rolling_count",
                 "pp_rolling_fill_ws_bytes", "pp_rolling_fill")
SHIMS = ("rolling_group", "rolling_bounds", "rolling_count", "rolling_fill")


class Stream:
    """What RollingTimeWindow reads of a TemporalGraph (which cannot be built without a device), over host tensors; ``to_static_graph`` is the
    brute force and counts its calls."""

    def __init__(self, edge_index, time, num_nodes):
        self.data = Data(edge_index=torch.as_tensor(edge_index), time=torch.as_tensor(time), num_nodes=num_nodes)
        self.mapping = IndexMap()
        self.calls = []

    @property
    def start_time(self):
        return self.data.time[0].item() if self.data.time.numel() else None

    @property
    def end_time(self):
        return self.data.time[-1].item() if self.data.time.numel() else None

    def to_static_graph(self, weighted=False, time_window=None):
        self.calls.append((weighted, time_window))
        index, weight, n = ops.brute_force(self.data.edge_index.numpy(), self.data.time.numpy(), time_window)
        data = Data(edge_index=torch.from_numpy(index), num_nodes=n, node_sequence=torch.arange(n).reshape(-1, 1))
        if weighted:
            data.edge_weight = torch.from_numpy(weight)
        return Graph(data, self.mapping, _row_sorted=True)


def same_as_brute_force(stream, graph, window):
    index, weight, n = ops.brute_force(stream.data.edge_index.numpy(), stream.data.time.numpy(), window)
    d = graph.data
    assert d.edge_index.dtype == torch.int64 and d.edge_weight.dtype == torch.float32
    assert np.array_equal(d.edge_index.numpy(), index), window
    assert np.array_equal(d.edge_weight.numpy(), weight), window
    assert d.num_nodes == n and graph.n == n and graph.mapping is stream.mapping
    assert d.node_sequence.tolist() == [[i] for i in range(n)] and graph.order == 1


@pytest.fixture
def restated(monkeypatch):
    ops.install(monkeypatch)
    reads = []
    read = rtw._read_report
    monkeypatch.setattr(rtw, "_read_report", lambda report: reads.append(1) or read(report))
    return reads


# ------------------------------------------------------------------ the algorithm, against brute force
@pytest.mark.parametrize("seed", range(24))
def test_restatement_reproduces_every_window_of_random_streams(restated, seed):
    rng = np.random.default_rng(seed)
    floats = seed % 3 == 2
    m, n, span = int(rng.integers(1, 120)), int(rng.choice([1, 2, 5, 40, 70000])), int(rng.integers(1, 60))
    ei, t = ops.random_stream(rng, m, n, span, floats)
    size = int(rng.integers(1, 25))
    step = int(rng.integers(1, 25))                      # below the size: overlaps; above: gaps; short spans: ties; sparse times: empty windows
    if floats:
        size, step = size / 4.0, step / 8.0 + 0.125
    stream = Stream(ei, t, n)
    batch = pp.algorithms.rolling_static_graphs(stream, size, step)
    assert batch is not None and restated == [1]
    windows, _ = rtw.schedule(stream.start_time, stream.end_time, size, step)
    assert batch.windows == windows and len(batch) == len(windows) >= 1
    assert batch.win_ptr.tolist() == list(batch.win_ptr_host) and batch.win_ptr.dtype == torch.int64
    assert batch.edge_index.shape == (2, batch.win_ptr_host[-1]) and batch.edge_weight.shape == (batch.win_ptr_host[-1],)
    assert all(isinstance(x, int) for x in batch.num_nodes)
    for i, window in enumerate(windows):
        same_as_brute_force(stream, batch.graph(i), window)
    assert stream.calls == []


def test_keys_are_32_bit_while_both_indices_fit_16_bits():
    assert _hip.rolling_key_dtype(1) == _hip.rolling_key_dtype(2) == _hip.rolling_key_dtype(65536) == torch.int32
    assert _hip.rolling_key_dtype(65537) == torch.int64
    handle = _lib.lib()
    for n in (0, 1, 2, 3, 65536, 65537, 1 << 31):
        assert handle.pp_rolling_key_bytes(n) == torch.empty(0, dtype=_hip.rolling_key_dtype(n)).element_size(), n
        assert ops.key_bits(n) * 2 <= 8 * handle.pp_rolling_key_bytes(n)


def test_restatement_with_the_largest_16_bit_indices(restated):
    ei = np.array([[65535, 65535, 0, 65535], [65535, 0, 65535, 65535]])
    stream = Stream(ei, np.array([1, 2, 3, 4]), 65536)
    batch = pp.algorithms.rolling_static_graphs(stream, 3, 1)
    assert batch.edge_index.dtype == torch.int64
    for i, window in enumerate(batch.windows):
        same_as_brute_force(stream, batch.graph(i), window)


# ------------------------------------------------------------------ schedule
def test_schedule_is_repeated_addition():
    windows, after = rtw.schedule(1, 50, 10, 10)
    assert windows == [(1, 11), (11, 21), (21, 31), (31, 41), (41, 51)] and after == 51
    windows, after = rtw.schedule(0.0, 1.0, 0.25, 0.1)
    t, want = 0.0, []
    while t <= 1.0:
        want.append((t, t + 0.25))
        t += 0.1
    assert windows == want and after == t
    assert [w[0] for w in windows] != [0.0 + i * 0.1 for i in range(len(windows))]          # 0.1 added three times is not 3 * 0.1
    assert len(windows) == 11                              # 0.1 added ten times is 0.9999999999999999 <= 1.0


def test_last_window_may_start_exactly_at_the_end_time():
    windows, after = rtw.schedule(0, 20, 5, 10)
    assert windows == [(0, 5), (10, 15), (20, 25)] and after == 30
    windows, after = rtw.schedule(0, 19, 5, 10)
    assert windows == [(0, 5), (10, 15)] and after == 20
    assert rtw.schedule(5, 4, 1, 1) == ([], 5)


def test_schedule_refuses_a_step_that_does_not_advance():
    assert rtw.schedule(1e17, 2e17, 1.0, 1.0) is None
    assert rtw.schedule(0.0, 3.0, 1.0, 1.0) == ([(0.0, 1.0), (1.0, 2.0), (2.0, 3.0), (3.0, 4.0)], 4.0)


# ------------------------------------------------------------------ iteration
REFERENCE_EXAMPLE = [("a", "b", 1), ("b", "c", 5), ("c", "d", 9), ("c", "e", 9), ("c", "f", 11), ("f", "a", 13), ("a", "g", 18), ("b", "f", 21),
                     ("a", "g", 26), ("c", "f", 27), ("h", "f", 27), ("g", "h", 28), ("a", "c", 30), ("a", "b", 31), ("c", "h", 32), ("f", "h", 33),
                     ("b", "i", 42), ("i", "b", 42), ("c", "i", 47), ("h", "i", 50)]


def example_stream():
    ids = "abcdefghi"
    ei = np.array([[ids.index(u) for u, _, _ in REFERENCE_EXAMPLE], [ids.index(v) for _, v, _ in REFERENCE_EXAMPLE]])
    return Stream(ei, np.array([t for _, _, t in REFERENCE_EXAMPLE]), 9)


def test_reference_example_and_stop_iteration(restated, monkeypatch):
    stream = example_stream()
    monkeypatch.setattr(stream, "to_static_graph", lambda *a, **k: pytest.fail("per-window call on the native path"))
    r = pp.algorithms.RollingTimeWindow(stream, 10, 10, return_window=True)
    assert iter(r) is r and r.current_time == 1 and (r.window_size, r.step_size, r.return_window, r.weighted, r.g) == (10, 10, True, True, stream)
    items = list(r)
    assert [w for _, w in items] == [(1, 11), (11, 21), (21, 31), (31, 41), (41, 51)]
    assert [g.data.edge_index.size(1) for g, _ in items] == [4, 3, 6, 3, 4]
    assert [g.n for g, _ in items] == [5, 7, 8, 8, 9]
    for g, w in items:
        same_as_brute_force(stream, g, w)
    assert r.current_time == 51 and restated == [1]
    for _ in range(2):
        with pytest.raises(StopIteration):
            next(r)
    assert restated == [1]
    plain = pp.algorithms.RollingTimeWindow(stream, 10, 10)
    assert isinstance(next(plain), Graph) and plain.current_time == 11


def test_groups_under_a_small_budget_and_a_window_above_it(restated, monkeypatch):
    rng = np.random.default_rng(5)
    ei, t = ops.random_stream(rng, 150, 6, 40)
    stream = Stream(ei, t, 6)
    monkeypatch.setattr(rtw, "BATCH_EDGES", 20)
    fills = []
    fill = _hip.rolling_fill
    monkeypatch.setattr(_hip, "rolling_fill", lambda *a, **k: fills.append((a[5], a[6], a[8])) or fill(*a, **k))
    r = pp.algorithms.RollingTimeWindow(stream, 9, 4, return_window=True)
    items = list(r)
    windows, _ = rtw.schedule(stream.start_time, stream.end_time, 9, 4)
    assert [w for _, w in items] == windows and restated == [1] and stream.calls == []
    for g, w in items:
        same_as_brute_force(stream, g, w)
    counts = [g.data.edge_index.size(1) for g, _ in items]
    assert max(counts) > 20 and len(fills) > 2                                       # at least one window alone above the budget
    assert [(a, b) for a, b, _ in fills] == rtw.window_groups(counts, 20)
    assert all(total == sum(counts[a:b]) and (total <= 20 or b == a + 1) for a, b, total in fills)
    # the batched entry point fills the same groups into one pair of buffers
    del fills[:]
    batch = pp.algorithms.rolling_static_graphs(stream, 9, 4)
    assert [(a, b) for a, b, _ in fills] == rtw.window_groups(counts, 20) and batch.win_ptr_host[-1] == sum(counts)
    for i, w in enumerate(windows):
        same_as_brute_force(stream, batch.graph(i), w)


def test_window_groups_are_greedy():
    assert rtw.window_groups([], 10) == []
    assert rtw.window_groups([3, 3, 3, 3], 10) == [(0, 3), (3, 4)]
    assert rtw.window_groups([3, 3, 4, 1], 10) == [(0, 3), (3, 4)]
    assert rtw.window_groups([11, 1, 25, 0, 0, 9, 2], 10) == [(0, 1), (1, 2), (2, 3), (3, 6), (6, 7)]
    assert rtw.window_groups([0, 0, 0], 1) == [(0, 3)]
    assert rtw.BATCH_EDGES == 1 << 27 and rtw._budget() == 1 << 27 < _hip._INT32_ROWS


def test_assigning_current_time_replans_from_the_new_value(restated):
    stream = example_stream()
    r = pp.algorithms.RollingTimeWindow(stream, 10, 10, return_window=True)
    assert next(r)[1] == (1, 11) and r.current_time == 11
    r.current_time = 25
    g, w = next(r)
    assert w == (25, 35) and restated == [1, 1]
    same_as_brute_force(stream, g, w)
    assert [w for _, w in r] == [(35, 45), (45, 55)] and r.current_time == 55 and restated == [1, 1]
    r.current_time = 50
    assert next(r)[1] == (50, 60) and restated == [1, 1, 1]
    with pytest.raises(StopIteration):
        next(r)
    assert stream.calls == []


def test_a_stream_without_events_yields_nothing():
    stream = Stream(np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64), 0)
    assert list(pp.algorithms.RollingTimeWindow(stream, 5)) == []
    assert pp.algorithms.rolling_static_graphs(stream, 5) is None


# ------------------------------------------------------------------ eligibility and fallback
def test_eligibility_decisions(monkeypatch):
    ints, floats = example_stream(), example_stream()
    floats.data.time = floats.data.time.to(torch.float64)
    assert not rtw.eligible(ints, 10, 10)                                            # host tensors
    monkeypatch.setattr(rtw, "_on_device", lambda edge_index, time: True)
    assert rtw.eligible(ints, 10, 10) and rtw.eligible(ints, 10, 3) and rtw.eligible(ints, 0, 1) and rtw.eligible(ints, -2, 1)
    assert not rtw.eligible(ints, 10, 10, weighted=False)
    assert not rtw.eligible(ints, 10.0, 10) and not rtw.eligible(ints, 10, 2.5) and not rtw.eligible(ints, np.int64(10), 10)
    assert not rtw.eligible(ints, 10, 0) and not rtw.eligible(ints, 10, -1) and not rtw.eligible(ints, True, 1)
    assert rtw.eligible(floats, 10, 10) and rtw.eligible(floats, 2.5, 0.1) and rtw.eligible(floats, 10, 0.5)
    assert not rtw.eligible(floats, float("nan"), 1.0) and not rtw.eligible(floats, 1.0, float("inf")) and not rtw.eligible(floats, 1.0, 0.0)
    assert not rtw.eligible(floats, 1.0, np.float32(1.0))
    narrow = example_stream()
    narrow.data.time = narrow.data.time.to(torch.int32)
    assert not rtw.eligible(narrow, 10, 10)
    single = example_stream()
    single.data.time = single.data.time.to(torch.float32)
    assert not rtw.eligible(single, 10, 10)
    monkeypatch.setattr(_hip, "_INT32_ROWS", 20)
    assert not rtw.eligible(ints, 10, 10)                                            # m < _INT32_ROWS
    monkeypatch.setattr(_hip, "_INT32_ROWS", 21)
    assert rtw.eligible(ints, 10, 10)
    monkeypatch.setattr(rtw, "NATIVE", False)
    assert not rtw.eligible(ints, 10, 10)


def reference_items(stream, size, step, weighted):
    out, t = [], stream.start_time
    while t <= stream.end_time:
        out.append((t, t + size))
        t += step
    return out


@pytest.mark.parametrize("case", ["unweighted", "float step on integer times", "switched off", "host tensors"])
def test_fallbacks_make_the_per_window_call(monkeypatch, case):
    for name in SHIMS:
        monkeypatch.setattr(_hip, name, lambda *a, **k: pytest.fail("a kernel wrapper was called on a fallback path"))
    if case != "host tensors":
        monkeypatch.setattr(rtw, "_on_device", lambda edge_index, time: True)
    if case == "switched off":
        monkeypatch.setattr(rtw, "NATIVE", False)
    assert rtw.NATIVE is (case != "switched off")
    stream = example_stream()
    size, step, weighted = (10, 2.5, True) if case.startswith("float") else (10, 7, case != "unweighted")
    r = pp.algorithms.RollingTimeWindow(stream, size, step, return_window=True, weighted=weighted)
    items = list(r)
    windows = reference_items(stream, size, step, weighted)
    assert [w for _, w in items] == windows and stream.calls == [(weighted, w) for w in windows]
    assert all(("edge_weight" in g.data) is weighted for g, _ in items)
    assert case == "unweighted" or pp.algorithms.rolling_static_graphs(stream, size, step) is None


@pytest.mark.parametrize("case", ["unsorted", "nan", "index", "long run"])
def test_what_the_device_finds_sends_the_iterator_to_the_per_window_call(restated, monkeypatch, case):
    stream = example_stream()
    size = step = 10
    if case == "unsorted":
        stream.data.time[3], stream.data.time[4] = 11, 9
    elif case == "nan":
        stream.data.time = stream.data.time.to(torch.float64)
        stream.data.time[5] = float("nan")
    elif case == "index":
        stream.data.num_nodes = 8                                                    # node 8 ("i") lies outside
    else:
        monkeypatch.setattr(rtw, "MAX_RUN", 2)                                       # ("a", "b") and ("a", "g") occur twice
    assert pp.algorithms.rolling_static_graphs(stream, size, step) is None and restated == [1]
    r = pp.algorithms.RollingTimeWindow(stream, size, step, return_window=True)
    first = next(r)
    assert first[1] == (stream.start_time, stream.start_time + 10) and stream.calls == [(True, first[1])] and restated == [1, 1]
    next(r)
    assert len(stream.calls) == 2 and restated == [1, 1]                             # decided once
    monkeypatch.setattr(rtw, "MAX_RUN", 3)
    if case == "long run":
        assert pp.algorithms.rolling_static_graphs(stream, size, step) is not None


# ------------------------------------------------------------------ library surface
def test_header_declares_and_library_exports_the_rolling_functions():
    protos = _lib.declared_functions()
    text = re.sub(r"/\*.*?\*/", " ", _lib.HEADER.read_text(), flags=re.S)
    handle = _lib.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
        restype, argtypes = protos[name]
        fn = getattr(handle, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    # the size queries are pure host code: keys + sort buffers per event; scan, two {window, position} pairs and sort buffers per edge
    assert handle.pp_rolling_group_ws_bytes(1 << 20, 1 << 20) >= (8 + 8 + 4) << 20
    assert handle.pp_rolling_group_ws_bytes(1 << 20, 1 << 16) >= (4 + 4 + 4) << 20
    assert handle.pp_rolling_fill_ws_bytes(1 << 20, 1 << 22) >= (4 << 20) + (16 + 8 << 22)
    for name in SHIMS:
        assert callable(getattr(_hip, name))
    assert (_hip.ROLLING_BAD_INDEX, _hip.ROLLING_BAD_ORDER, _hip.ROLLING_LONG_RUN) == (ops.BAD_INDEX, ops.BAD_ORDER, ops.LONG_RUN) == (1, 2, 4)
    assert pp.algorithms.RollingTimeWindow is rtw.RollingTimeWindow and pp.algorithms.rolling_static_graphs is rtw.rolling_static_graphs
    assert pp.algorithms.RollingWindows is rtw.RollingWindows and rtw.MAX_RUN == 1 << 24
