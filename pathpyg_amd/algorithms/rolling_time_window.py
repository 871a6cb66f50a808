"""Rolling time windows over a temporal graph, API-compatible with ``pathpyG.algorithms.RollingTimeWindow`` (reference
src/pathpyG/algorithms/rolling_time_window.py:4-61).

The reference calls ``TemporalGraph.to_static_graph(weighted, time_window)`` once per window: two masks over all ``m`` events, a compaction,
a read-back and a full sort-and-merge each time.  Here the weighted graphs of ALL windows come out of one pass (csrc/pp_rolling.hip): the
events are grouped by node pair once, a window is a range of the time-sorted events, and which pairs a window holds — and how often —
follows from event ranks alone.  :func:`rolling_static_graphs` is that batched pass; :class:`RollingTimeWindow` iterates over its result
and yields, window for window, exactly what the per-window call returns.  Streams the pass does not take (see :func:`eligible`) go
through the per-window call as in the reference.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from .. import _hip
from ..core.graph import Graph
from ..data import Data, Lazy

NATIVE = True                 # False: RollingTimeWindow always calls to_static_graph per window and rolling_static_graphs returns None
BATCH_EDGES = 1 << 27         # edges of all windows of one fill-and-sort group (a single larger window is a group of its own)
MAX_RUN = 1 << 24             # events of one node pair from which a float32 sum of ones and a converted count may differ
# Largest number of windows a plan enumerates.  A plan spends host memory per window: the (start, end) tuple in `windows` (56 bytes), its
# two Python numbers (24 to 32 bytes each) and its list slot (8); a slot each in `starts` and `ends` (16); lo and hi (8 together), the
# report (4) and win_ptr (8) — about 160 bytes, 200 with the temporaries of the running sums.  2^22 windows are 0.8 GiB, so a plan
# stays below 1 GiB.  Longer schedules, and an infinite last timestamp (which has no last window), go window by window, lazily, as in the
# reference.  Must not exceed _hip._INT32_ROWS, the kernels' own limit.
MAX_WINDOWS = 1 << 22

_INT64 = (-(1 << 63), (1 << 63) - 1)


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


def _is_number(x) -> bool:
    return (isinstance(x, float) and math.isfinite(x)) or _is_int(x)


def _on_device(edge_index: torch.Tensor, time: torch.Tensor) -> bool:
    return edge_index.is_cuda and time.device == edge_index.device


def eligible(g, window_size, step_size, weighted: bool = True) -> bool:
    """Whether the batched pass can take this stream, as far as that shows without looking at the events: weighted graphs, events on a
    CUDA device, fewer than 2^31 - 16 of them, and a window arithmetic that torch carries out in the time tensor's own dtype — int64 times
    with ``int`` window and step, or float64 times with finite Python numbers — with a positive step.  (Sortedness, NaN timestamps, node
    indices outside the graph and pairs of ``MAX_RUN`` events or more are found on the device and reported with the window counts.)"""
    if not (NATIVE and weighted):
        return False
    ei, time = g.data.edge_index, g.data.time
    if not (isinstance(ei, torch.Tensor) and isinstance(time, torch.Tensor) and _on_device(ei, time)):
        return False
    m = time.numel()
    if m == 0 or m >= _hip._INT32_ROWS or ei.dim() != 2 or ei.size(0) != 2 or ei.size(1) != m or ei.dtype != torch.int64:
        return False
    n = g.data.num_nodes
    if not _is_int(n) or not 0 < n <= 1 << 31:
        return False
    if time.dtype == torch.int64:
        numbers = _is_int(window_size) and _is_int(step_size)
    elif time.dtype == torch.float64:
        numbers = _is_number(window_size) and _is_number(step_size)
    else:
        numbers = False
    return numbers and step_size > 0


def schedule(start, end_time, window_size, step_size, limit=None):
    """The reference's windows from ``start`` on (rolling_time_window.py:52-55): ``(t, t + window_size)`` while ``t <= end_time``, ``t``
    advanced by REPEATED addition of the step.  Returns ``(windows, next)`` with ``next`` the first start beyond ``end_time`` — or ``None``
    when a step no longer changes ``t`` (a float step below the spacing of the times: the reference then yields one window for ever), or
    when there are more than ``limit`` windows: integer schedules are counted before the first one is made, float schedules (whose count
    only the additions themselves give) stop at window ``limit + 1``."""
    if limit is not None and _is_int(start) and _is_int(end_time) and _is_int(step_size) and step_size > 0 \
            and start <= end_time and (end_time - start) // step_size + 1 > limit:
        return None
    windows, t = [], start
    while t <= end_time:
        if limit is not None and len(windows) >= limit:
            return None
        windows.append((t, t + window_size))
        if t + step_size == t:
            return None
        t += step_size
    return windows, t


def window_groups(counts, budget: int) -> list[tuple[int, int]]:
    """Consecutive windows cut greedily into groups ``(w0, w1)`` of at most ``budget`` edges each; one window above the budget stands alone."""
    groups, w0, held = [], 0, 0
    for w, c in enumerate(counts):
        if w > w0 and held + int(c) > budget:
            groups.append((w0, w))
            w0, held = w, 0
        held += int(c)
    if len(counts) > w0:
        groups.append((w0, len(counts)))
    return groups


def _budget() -> int:
    return max(1, min(int(BATCH_EDGES), _hip._INT32_ROWS - 1))


def _read_report(report: torch.Tensor) -> np.ndarray:
    """The one read-back of a plan: the difference array of the per-window edge counts and the status word."""
    return report.cpu().numpy()


class RollingWindows:
    """The weighted static graphs of consecutive windows in one batch: window ``i`` owns the columns ``win_ptr[i] .. win_ptr[i + 1] - 1`` of
    ``edge_index`` (int64 ``[2, total]``, (source, target)-sorted inside a window) and ``edge_weight`` (float32 ``[total]``, the number of the
    pair's events in the window); ``num_nodes[i]`` is its largest node index + 1 (0 for an empty window) and ``windows[i]`` its
    ``(start, end)``.  ``win_ptr_host`` is the host copy of ``win_ptr``."""

    def __init__(self, windows, win_ptr_host, edge_index, edge_weight, num_nodes, mapping):
        self.windows = windows
        self.win_ptr_host = win_ptr_host
        self.win_ptr = torch.from_numpy(np.ascontiguousarray(win_ptr_host)).to(edge_index.device)
        self.edge_index, self.edge_weight, self.num_nodes, self.mapping = edge_index, edge_weight, num_nodes, mapping

    def __len__(self) -> int:
        return len(self.windows)

    def graph(self, i: int) -> Graph:
        """Window ``i`` as a :class:`Graph` over views of the batch (what ``to_static_graph(weighted=True, time_window=windows[i])`` returns);
        no kernel runs and nothing is read back."""
        a, b, n = int(self.win_ptr_host[i]), int(self.win_ptr_host[i + 1]), self.num_nodes[i]
        dev = self.edge_index.device
        data = Data(edge_index=self.edge_index[:, a:b], edge_weight=self.edge_weight[a:b], num_nodes=n,
                    node_sequence=Lazy(lambda: torch.arange(n, device=dev).reshape(-1, 1), (n, 1)))
        return Graph(data, self.mapping, _row_sorted=True)


class _Plan(NamedTuple):
    g: object
    windows: list              # (start, end) per window
    starts: list               # W + 1 starts: starts[i + 1] is where the reference's current_time stands after window i
    grouping: tuple            # (keys, perm, flags) of pp_rolling_group
    lo: torch.Tensor
    hi: torch.Tensor
    win_ptr: np.ndarray        # int64 [W + 1], host
    cnt: object                # rolling_count's per-position counts over ALL windows while one group holds them, else None


def _plan(g, window_size, step_size, start_time=None, grouping=None):
    """Windows, their event ranges and their edge counts — one read-back.  ``None``: the stream is not eligible, or its schedule has more
    than ``MAX_WINDOWS`` windows or no end (decided before any window is enumerated on integer times, at window ``MAX_WINDOWS + 1`` on
    float times)."""
    if not eligible(g, window_size, step_size):
        return None
    time = g.data.time
    integer = time.dtype == torch.int64
    bounds = time[[0, -1]].tolist()
    start, end_time = (bounds[0] if start_time is None else start_time), bounds[1]
    if not (_is_int(start) if integer else _is_number(start)) or not (integer or math.isfinite(end_time)):
        return None                 # (a NaN or infinite last timestamp: no schedule ends there)
    planned = schedule(start, end_time, window_size, step_size, min(int(MAX_WINDOWS), _hip._INT32_ROWS - 1))
    if planned is None:
        return None
    windows, after = planned
    W = len(windows)
    starts = [w[0] for w in windows] + [after]
    ends = [w[1] for w in windows]
    if W == 0:                      # the start lies beyond the last event already
        return _Plan(g, windows, starts, grouping, None, None, np.zeros(1, dtype=np.int64), None)
    if integer and W and not (_INT64[0] <= min(starts[0], ends[0]) and max(starts[-1], ends[-1]) <= _INT64[1]):
        return None
    dev = time.device
    if grouping is None:
        grouping = _hip.rolling_group(g.data.edge_index, time, g.data.num_nodes)
    keys, perm, flags = grouping
    lo, hi = _hip.rolling_bounds(time, torch.tensor(starts[:W], dtype=time.dtype, device=dev), torch.tensor(ends, dtype=time.dtype, device=dev))
    cnt, report = _hip.rolling_count(keys, perm, lo, hi, 0, W, MAX_RUN, flags)
    report = _read_report(report)
    if report[W + 1] != 0:
        return None
    win_ptr = np.zeros(W + 1, dtype=np.int64)
    np.cumsum(np.cumsum(report[:W], dtype=np.int64), out=win_ptr[1:])
    if len(window_groups(np.diff(win_ptr), _budget())) > 1:
        cnt = None
    return _Plan(g, windows, starts, grouping, lo, hi, win_ptr, cnt)


def _build(plan: _Plan, w0: int, w1: int) -> RollingWindows:
    """The windows ``w0 .. w1 - 1`` of a plan as one batch: fill and window sort group by group into one pair of buffers, then one read-back
    of the windows' node counts."""
    keys, perm, flags = plan.grouping or (None, None, None)            # (a plan without windows may have no grouping)
    dev = plan.g.data.time.device
    ptr = plan.win_ptr
    total = int(ptr[w1] - ptr[w0])
    W = len(plan.windows)
    index = torch.empty((2, total), dtype=torch.int64, device=dev)
    weight = torch.empty(total, dtype=torch.float32, device=dev)
    parts = []
    for a, b in window_groups(np.diff(ptr[w0:w1 + 1]), _budget()):
        a, b = a + w0, b + w0
        if plan.cnt is not None and (a, b) == (0, W):
            cnt = plan.cnt
        else:
            cnt, _ = _hip.rolling_count(keys, perm, plan.lo, plan.hi, a, b, MAX_RUN, flags)
        parts.append(_hip.rolling_fill(keys, perm, plan.g.data.num_nodes, plan.lo, plan.hi, a, b, cnt, int(ptr[b] - ptr[a]),
                                       out=(index, weight, int(ptr[a] - ptr[w0])))[2])
    # (the node counts are unsigned 32-bit words in an int32 tensor: node 2^31 - 1 makes a window of 2^31 nodes)
    num_nodes = (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy().view(np.uint32).tolist() if parts else []
    return RollingWindows(plan.windows[w0:w1], ptr[w0:w1 + 1] - ptr[w0], index, weight, num_nodes, plan.g.mapping)


def rolling_static_graphs(g, window_size, step_size=1, start_time=None) -> RollingWindows | None:
    """The weighted static graphs of all windows ``[t, t + window_size)`` of the temporal graph ``g``, ``t`` running from ``start_time``
    (default ``g.start_time``) in steps of ``step_size`` while ``t <= g.end_time``, as one :class:`RollingWindows` batch.  ``None`` when the
    stream is not eligible for the batched pass (:func:`eligible`; a schedule of more than ``MAX_WINDOWS`` windows, which is refused
    before it is enumerated, or one that never ends: an infinite last timestamp, a step that does not advance; or what the device found:
    unsorted or NaN times, a node index outside the graph, a node pair with ``MAX_RUN`` events or more) — iterate a
    :class:`RollingTimeWindow` then, which goes window by window and lazily."""
    plan = _plan(g, window_size, step_size, start_time)
    if plan is None:
        return None
    return _build(plan, 0, len(plan.windows))


class RollingTimeWindow:
    """An iterable rolling time window for time-slice analysis of a temporal graph (reference rolling_time_window.py:4-61): yields the
    static graph of ``[current_time, current_time + window_size)`` — or ``(graph, (start, end))`` with ``return_window`` — and advances
    ``current_time`` by ``step_size`` until it passes the last timestamp.

    On eligible streams the graphs come from :func:`rolling_static_graphs`' pass, built lazily at the first ``__next__`` in groups of
    consecutive windows of at most ``BATCH_EDGES`` edges; assigning ``current_time`` between two ``__next__`` calls re-plans from the new
    value.  Otherwise every ``__next__`` calls ``to_static_graph`` as the reference does."""

    def __init__(self, temporal_graph, window_size, step_size=1, return_window=False, weighted=True):
        self.g = temporal_graph
        self.window_size = window_size
        self.step_size = step_size
        self.current_time = self.g.start_time
        self.return_window = return_window
        self.weighted = weighted
        self._native = None            # None: not decided yet
        self._plan = None
        self._grouping = None
        self._groups = []
        self._batch, self._batch_range = None, (0, 0)
        self._next, self._expected = 0, None

    def __iter__(self):
        return self

    def _replan(self) -> bool:
        self._plan = _plan(self.g, self.window_size, self.step_size, self.current_time, self._grouping)
        if self._plan is None:
            return False
        self._grouping = self._plan.grouping
        self._groups = window_groups(np.diff(self._plan.win_ptr), _budget())
        self._batch, self._batch_range, self._next = None, (0, 0), 0
        return True

    def _next_native(self):
        if self._plan is None or self.current_time != self._expected or type(self.current_time) is not type(self._expected):
            if not self._replan():
                self._native = False
                return None
        plan, i = self._plan, self._next
        if i >= len(plan.windows):
            raise StopIteration()
        if not self._batch_range[0] <= i < self._batch_range[1]:
            self._batch = None                                  # (the previous group's buffers go before the next ones come)
            self._batch_range = next(r for r in self._groups if r[0] <= i < r[1])
            self._batch = _build(plan, *self._batch_range)
        graph = self._batch.graph(i - self._batch_range[0])
        self._next = i + 1
        self.current_time = self._expected = plan.starts[i + 1]
        return (graph, plan.windows[i]) if self.return_window else graph

    def __next__(self):
        if self.g.data.time.numel() == 0:
            raise StopIteration()
        if self._native is None:
            self._native = eligible(self.g, self.window_size, self.step_size, self.weighted)
        if self._native:
            item = self._next_native()
            if item is not None:
                return item
        if self.current_time <= self.g.end_time:
            time_window = (self.current_time, self.current_time + self.window_size)
            s = self.g.to_static_graph(weighted=self.weighted, time_window=time_window)
            self.current_time += self.step_size
            if self.return_window:
                return s, time_window
            return s
        raise StopIteration()
