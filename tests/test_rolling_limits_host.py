"""RollingTimeWindow at its limits, host side (algorithms/rolling_time_window.py over the numpy restatement tests/cpu_ops_rolling.py): the
window schedule is bounded by ``MAX_WINDOWS`` and refused before it is enumerated, an infinite last timestamp is refused, and in both cases
the iterator goes window by window, lazily; infinite and extreme timestamps that the batched pass does take; and the restatement at the
node index limits (one node, both 16-bit halves full, the first 64-bit key width, node 2^31 - 1 whose window has 2^31 nodes).  Everything is
exact.  No GPU.  ``INDEX_CASES`` and ``windows_of`` are shared with tests/test_gpu_rolling_limits.py, which runs them on the kernels."""
import math

import numpy as np
import pytest
import torch

import cpu_ops_rolling as ops
import pathpyg_amd as pp
from pathpyg_amd import _hip
from pathpyg_amd.algorithms import rolling_time_window as rtw
from test_rolling_host import Stream, restated, same_as_brute_force  # noqa: F401  (restated is a fixture)

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1


def tiny_stream(times, n=3):
    m = len(times)
    ei = np.array([[i % n for i in range(m)], [(i + 1) % n for i in range(m)]], dtype=np.int64)
    return Stream(ei, np.asarray(times), n)


def reference_windows(start, end_time, size, step, at_most=None):
    """The reference's loop (rolling_time_window.py:52-55), cut off after ``at_most`` windows."""
    out, t = [], start
    while t <= end_time and (at_most is None or len(out) < at_most):
        out.append((t, t + size))
        t += step
    return out


# ------------------------------------------------------------------ A1: the schedule is bounded
def test_the_window_cap_is_documented_and_below_the_kernels_limit():
    """About 200 bytes of host memory per window (see the comment at the constant): 2^22 windows stay below 1 GiB."""
    assert rtw.MAX_WINDOWS == 1 << 22 and rtw.MAX_WINDOWS <= _hip._INT32_ROWS
    assert rtw.MAX_WINDOWS * 200 < 1 << 30
    assert "MAX_WINDOWS" in rtw.rolling_static_graphs.__doc__


@pytest.mark.parametrize("step", [1, 3])
def test_integer_schedules_at_the_cap(restated, monkeypatch, step):
    monkeypatch.setattr(rtw, "MAX_WINDOWS", 1000)
    exact = tiny_stream([0, 5 * step, 999 * step])                     # starts 0, step, ..., 999 * step: exactly 1000 windows
    batch = pp.algorithms.rolling_static_graphs(exact, 2 * step, step)
    assert batch is not None and len(batch) == 1000 and restated == [1] and exact.calls == []
    assert batch.windows == reference_windows(0, 999 * step, 2 * step, step)
    for i in (0, 1, 4, 5, 6, 998, 999):
        same_as_brute_force(exact, batch.graph(i), batch.windows[i])
    r = pp.algorithms.RollingTimeWindow(exact, 2 * step, step)
    assert len(list(r)) == 1000 and exact.calls == [] and restated == [1, 1]


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("windows", [1001, 100_001])
def test_integer_schedules_above_the_cap_are_refused_unenumerated(restated, monkeypatch, step, windows):
    monkeypatch.setattr(rtw, "MAX_WINDOWS", 1000)
    last = (windows - 1) * step
    assert len(range(0, last + 1, step)) == windows
    assert rtw.schedule(0, last, 2 * step, step, 1000) is None and rtw.schedule(0, last - step, 2 * step, step, windows - 1) is not None
    for name in ("rolling_group", "rolling_bounds", "rolling_count", "rolling_fill"):
        monkeypatch.setattr(_hip, name, lambda *a, **k: pytest.fail("a kernel wrapper ran for a refused schedule"))
    stream = tiny_stream([0, 5 * step, last])
    assert pp.algorithms.rolling_static_graphs(stream, 2 * step, step) is None and restated == [] and stream.calls == []
    # (the last window may start below the last timestamp: the count is floor((end - start) / step) + 1)
    assert rtw.schedule(0, 1000 * step - 1, step, step, 1000) is not None and rtw.schedule(0, 1000 * step, step, step, 1000) is None


def test_float_schedules_at_the_cap_count_by_repeated_addition(restated, monkeypatch):
    """Step 0.1: the count is what the reference's own additions give.  A thousand additions of 0.1 make 99.9999999999986, BELOW 100.0, so a
    stream that ends at 100.0 has the 1001 windows one expects — and so has one that ends exactly at that sum, while one that ends an ulp
    below it has 1000.  999 additions make 99.89999999999861 <= 99.9: 1000 windows."""
    monkeypatch.setattr(rtw, "MAX_WINDOWS", 1000)
    t1000 = 0.0
    for _ in range(1000):
        t1000 += 0.1
    assert t1000 == 99.9999999999986 and t1000 < 100.0 and t1000 != 1000 * 0.1
    t100000 = 0.0
    for _ in range(100_000):
        t100000 += 0.1
    assert t100000 > 10000.0                    # by then the sum has drifted ABOVE: a stream ending at 10000.0 has 100 000 windows, not 100 001
    sides = {99.9: 1000, math.nextafter(t1000, 0.0): 1000, t1000: 1001, 100.0: 1001, 10000.0: 100_000, t100000: 100_001}
    for end, count in sides.items():
        assert len(reference_windows(0.0, end, 0.25, 0.1)) == count, end
        stream = tiny_stream([0.0, 0.55, end])
        del restated[:]
        batch = pp.algorithms.rolling_static_graphs(stream, 0.25, 0.1)
        if count <= 1000:
            assert batch is not None and batch.windows == reference_windows(0.0, end, 0.25, 0.1) and restated == [1]
            for i in (0, 3, 4, 5, 6, 999):
                same_as_brute_force(stream, batch.graph(i), batch.windows[i])
        else:
            assert batch is None and restated == []
        assert stream.calls == []
    # the float loop stops when the list reaches the cap (10^14 additions would not end)
    assert rtw.schedule(0.0, 1e13, 0.25, 0.1, 1000) is None
    assert rtw.schedule(0.0, 99.9, 0.25, 0.1, 1000) is not None and rtw.schedule(0.0, 99.9, 0.25, 0.1, 999) is None


def first_three_lazily(stream, size, step):
    r = pp.algorithms.RollingTimeWindow(stream, size, step, return_window=True)
    items = [next(r) for _ in range(3)]
    want = reference_windows(stream.start_time, stream.end_time, size, step, at_most=3)
    assert [w for _, w in items] == want and len(want) == 3
    assert stream.calls == [(True, w) for w in want]                   # exactly three per-window calls: nothing ran ahead
    for g, w in items:
        same_as_brute_force(stream, g, w)
    assert r.current_time == want[-1][0] + step


def test_ten_to_the_thirteen_windows_are_refused_at_once_and_iterated_lazily(restated):
    """int64 times [0, 10^13] with window and step 1: 10^13 + 1 windows.  (Before the bound this call did not return: it appended tuples
    until memory ran out.)"""
    stream = tiny_stream(np.array([0, 1, 2, 10 ** 13], dtype=np.int64))
    assert (10 ** 13 - 0) // 1 + 1 > rtw.MAX_WINDOWS
    assert pp.algorithms.rolling_static_graphs(stream, 1, 1) is None and restated == [] and stream.calls == []
    first_three_lazily(stream, 1, 1)
    assert restated == []


def test_an_infinite_last_timestamp_is_refused_and_iterated_lazily(restated):
    """A float64 stream that ends in +inf: ``t <= inf`` holds for every finite t, the schedule has no last window.  (Before the fix the loop
    never ended: only a NaN end was caught.)"""
    stream = tiny_stream(np.array([0.0, 0.5, 1.0, 2.5, np.inf]))
    assert pp.algorithms.rolling_static_graphs(stream, 1.0, 1.0) is None and restated == [] and stream.calls == []
    first_three_lazily(stream, 1.0, 1.0)
    assert restated == []
    both = tiny_stream(np.array([-np.inf, np.inf]))                    # start and end infinite: the reference's one window for ever
    assert pp.algorithms.rolling_static_graphs(both, 1.0, 1.0) is None
    down = tiny_stream(np.array([-np.inf, -np.inf]))
    assert pp.algorithms.rolling_static_graphs(down, 1.0, 1.0) is None and pp.algorithms.rolling_static_graphs(down, 1.0, 1.0, 0.0) is None


# ------------------------------------------------------------------ A2: non-finite and extreme times that stay native
def test_leading_minus_infinity_events_are_in_no_window(restated):
    rng = np.random.default_rng(21)
    ei, t = ops.random_stream(rng, 60, 6, 40, floats=True)
    ei[:, :2] = [[7, 7], [8, 8]]                                       # the pair (7, 8) occurs at -inf only
    t[:2] = -np.inf
    assert (t[2:] >= 0.0).all()
    stream = Stream(ei, t, 9)
    batch = pp.algorithms.rolling_static_graphs(stream, 1.5, 1.5, start_time=0.0)
    assert batch is not None and restated == [1] and batch.windows == reference_windows(0.0, float(t[-1]), 1.5, 1.5) and len(batch) >= 5
    for i, w in enumerate(batch.windows):
        same_as_brute_force(stream, batch.graph(i), w)
    assert not ((batch.edge_index[0] == 7) | (batch.edge_index[1] == 8)).any()
    assert batch.edge_weight.sum().item() == 58 and max(batch.num_nodes) <= 6          # disjoint windows: every finite event once
    assert stream.calls == []
    # from the stream's own start, -inf, there is no schedule: `t + step == t`
    assert pp.algorithms.rolling_static_graphs(stream, 1.5, 1.5) is None


def test_int64_times_from_the_smallest_value_on(restated):
    t = np.array([I64_MIN, I64_MIN, I64_MIN + 3, I64_MIN + 4, I64_MIN + 9, I64_MIN + 17, I64_MIN + 20], dtype=np.int64)
    stream = tiny_stream(t)
    batch = pp.algorithms.rolling_static_graphs(stream, 7, 5)
    assert batch is not None and restated == [1] and stream.calls == []
    assert batch.windows == [(I64_MIN + 5 * i, I64_MIN + 5 * i + 7) for i in range(5)]
    for i, w in enumerate(batch.windows):
        same_as_brute_force(stream, batch.graph(i), w)
    # events 0..3 (pairs (0,1) (1,2) (2,0) (0,1)) | +9 | none in [+10, +17) | +17 and +20 | +20
    assert np.diff(batch.win_ptr_host).tolist() == [3, 1, 0, 2, 1]


def outcome(step_through):
    """Items of an iteration and the type of the exception that ended it (None: it ended by itself)."""
    items = []
    try:
        for item in step_through:
            items.append(item)
    except Exception as e:                                             # noqa: BLE001  (whatever the per-window call raises)
        return items, type(e)
    return items, None


def test_a_window_end_beyond_int64_goes_the_per_window_way(restated):
    t = np.array([I64_MAX - 20, I64_MAX - 13, I64_MAX - 12, I64_MAX - 4, I64_MAX], dtype=np.int64)
    stream, twin = tiny_stream(t), tiny_stream(t)
    assert reference_windows(I64_MAX - 20, I64_MAX, 7, 5)[-1] == (I64_MAX, I64_MAX + 7)          # the last window ends beyond int64
    assert pp.algorithms.rolling_static_graphs(stream, 7, 5) is None and restated == [] and stream.calls == []

    def loop():
        now = twin.start_time
        while now <= twin.end_time:
            yield twin.to_static_graph(weighted=True, time_window=(now, now + 7)), (now, now + 7)
            now += 5
    want, want_error = outcome(loop())
    got, got_error = outcome(pp.algorithms.RollingTimeWindow(stream, 7, 5, return_window=True))
    assert got_error is want_error and [w for _, w in got] == [w for _, w in want] and len(want) >= 3
    assert stream.calls == twin.calls
    for (g, _), (ref, _) in zip(got, want):
        assert torch.equal(g.data.edge_index, ref.data.edge_index) and torch.equal(g.data.edge_weight, ref.data.edge_weight) and g.n == ref.n
    # one step earlier everything fits: native
    fits = tiny_stream(t - 7)
    batch = pp.algorithms.rolling_static_graphs(fits, 7, 5)
    assert batch is not None and batch.windows[-1] == (I64_MAX - 7, I64_MAX)
    for i, w in enumerate(batch.windows):
        same_as_brute_force(fits, batch.graph(i), w)


# ------------------------------------------------------------------ A3 (and C3 of the device file): the node index limits
def index_stream(n, top):
    """At most 50 events over 12 time units with ``top`` the largest node: as source only (t 0..2), as target only (3..5), on both sides
    (6..8, three times, after two smaller pairs) and as the one edge of the window 9..11."""
    low, mid = 0, min(1, n - 1)
    events = [(top, low, 0), (mid, low, 0), (top, mid, 1), (top, low, 2), (low, low, 2),
              (low, top, 3), (mid, top, 4), (low, mid, 4), (low, top, 5),
              (mid, mid, 6), (top, top, 6), (low, top, 7), (top, top, 7), (top, top, 8), (top, low, 8),
              (top, top, 10)]
    ei = np.array([[u for u, _, _ in events], [v for _, v, _ in events]], dtype=np.int64)
    return ei, np.array([t for _, _, t in events], dtype=np.int64)


# name: (num_nodes, largest node)
INDEX_CASES = {
    "one node": (1, 0),
    "two nodes": (2, 1),
    "n = 65536: both 16-bit halves full": (65536, 65535),
    "n = 65537: the first 64-bit keys": (65537, 65536),
    "n = 2^31 - 1": (2 ** 31 - 1, 2 ** 31 - 2),
    "n = 2^31: a window of 2^31 nodes": (2 ** 31, 2 ** 31 - 1),
}
INDEX_SCHEDULES = [(3, 3), (5, 2)]                                     # (window, step): disjoint, and overlapping with the lone edge shared


def windows_of(mod, ei, t, n, windows, device="cpu", groups=None):
    """The four calls of the pass, made directly on ``mod`` (the restatement or ``_hip``): per window ``(edge_index, edge_weight,
    num_nodes)`` as numpy / int, and the status word."""
    ei_t, t_t = torch.as_tensor(ei).to(device), torch.as_tensor(t).to(device)
    keys, perm, flags = mod.rolling_group(ei_t, t_t, n)
    assert keys.dtype == _hip.rolling_key_dtype(n)
    W = len(windows)
    lo, hi = mod.rolling_bounds(t_t, torch.tensor([w[0] for w in windows], dtype=t_t.dtype, device=device),
                                torch.tensor([w[1] for w in windows], dtype=t_t.dtype, device=device))
    out = []
    status = 0
    for w0, w1 in groups or [(0, W)]:
        cnt, report = mod.rolling_count(keys, perm, lo, hi, w0, w1, 1 << 24, flags)
        report = report.cpu().numpy()
        status |= int(report[-1])
        counts = np.cumsum(report[:w1 - w0], dtype=np.int64)
        assert report[:w1 - w0 + 1].sum() == 0 and int(cnt.sum()) == counts.sum()
        index, weight, nn = mod.rolling_fill(keys, perm, n, lo, hi, w0, w1, cnt, int(counts.sum()))
        index, weight, nn = index.cpu().numpy(), weight.cpu().numpy(), nn.cpu().numpy()
        assert nn.dtype == np.int32 and index.dtype == np.int64 and weight.dtype == np.float32
        ptr = np.concatenate([[0], np.cumsum(counts)])
        for i in range(w1 - w0):
            out.append((index[:, ptr[i]:ptr[i + 1]], weight[ptr[i]:ptr[i + 1]], int(nn.view(np.uint32)[i])))
    return out, status


def check_index_case(mod, name, device="cpu"):
    n, top = INDEX_CASES[name]
    ei, t = index_stream(n, top)
    assert ei.shape[1] <= 50 and ei.max() == top == n - 1
    for size, step in INDEX_SCHEDULES:
        windows = reference_windows(0, 10, size, step)
        got, status = windows_of(mod, ei, t, n, windows, device)
        assert status == 0 and 4 <= len(got) <= 6
        alone = 0
        for (index, weight, nodes), w in zip(got, windows):
            want_index, want_weight, want_nodes = ops.brute_force(ei, t, w)
            assert np.array_equal(index, want_index) and np.array_equal(weight, want_weight), (name, w)
            assert nodes == want_nodes, (name, w, nodes, want_nodes)
            alone += want_index.shape[1] == 1 and want_index.max() == top
        assert alone >= 1                                              # a window whose only edge holds the largest node
        assert max(nodes for _, _, nodes in got) == n                  # (2^31 in the last case)


@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_restatement_at_the_node_index_limits(name):
    check_index_case(ops, name)


def test_key_width_flips_at_65537_nodes():
    assert _hip.rolling_key_dtype(65536) == torch.int32 and _hip.rolling_key_dtype(65537) == torch.int64
    assert ops.key_bits(65536) == 16 and ops.key_bits(65537) == 17 and ops.key_bits(1) == 1 and ops.key_bits(2) == 1
    assert ops.key_bits(2 ** 31 - 1) == ops.key_bits(2 ** 31) == 31


def test_a_window_of_two_to_the_31_nodes_through_the_package(restated):
    """Node 2^31 - 1 in a graph of 2^31 nodes, through planning, grouping and iteration: the item's node count is 2^31, not a wrapped 0 or
    -2^31.  (``Stream.to_static_graph`` would make a node_sequence of 2^31 rows, so the items are compared with ``ops.brute_force``.)"""
    n, top = INDEX_CASES["n = 2^31: a window of 2^31 nodes"]
    ei, t = index_stream(n, top)
    stream = Stream(ei, t, n)
    assert rtw.eligible(stream, 3, 3)
    batch = pp.algorithms.rolling_static_graphs(stream, 3, 3)
    assert batch is not None and len(batch) == 4 and batch.num_nodes == [2 ** 31] * 4 and all(type(x) is int for x in batch.num_nodes)
    for i, w in enumerate(batch.windows):
        want_index, want_weight, want_nodes = ops.brute_force(ei, t, w)
        g = batch.graph(i)
        assert np.array_equal(g.data.edge_index.numpy(), want_index) and np.array_equal(g.data.edge_weight.numpy(), want_weight)
        assert g.n == g.data.num_nodes == want_nodes == 2 ** 31
        assert g.data.peek("node_sequence").shape == (2 ** 31, 1)     # still unmade
    assert stream.calls == []
