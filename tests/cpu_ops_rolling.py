"""numpy restatement of the rolling-window kernels (csrc/pp_rolling.hip), with the arguments and results of the ``_hip.rolling_*`` wrappers
(torch tensors in and out, here on the host), and the brute force they are checked against: one mask + ``np.unique`` per window, which is
what ``TemporalGraph.to_static_graph(weighted=True, time_window=...)`` computes."""
import numpy as np
import torch

BAD_INDEX, BAD_ORDER, LONG_RUN = 1, 2, 4


def key_bits(num_nodes: int) -> int:
    return max(int(max(num_nodes, 2) - 1).bit_length(), 1)


def rolling_group(edge_index, time, num_nodes):
    ei, t, bits = edge_index.numpy(), time.numpy(), key_bits(num_nodes)
    m = ei.shape[1]
    flags = 0
    ok = (ei >= 0).all(0) & (ei < num_nodes).all(0)
    if not ok.all():
        flags |= BAD_INDEX
    if t.dtype.kind == "f" and np.isnan(t).any() or (m > 1 and (t[:-1] > t[1:]).any()):
        flags |= BAD_ORDER
    raw = np.where(ok, (ei[0].astype(np.uint64) << np.uint64(bits)) | ei[1].astype(np.uint64), np.uint64(0))
    perm = np.argsort(raw, kind="stable")
    dtype = np.int32 if 2 * bits <= 32 else np.int64
    return torch.from_numpy(raw[perm].astype(dtype)), torch.from_numpy(perm.astype(np.int32)), torch.tensor([flags], dtype=torch.int32)


def _unsigned(keys):
    """The keys as the kernels see them: unsigned words (an int32 tensor holds uint32 keys when both indices fit 16 bits)."""
    k = keys.numpy()
    return k.view(np.uint32 if k.dtype == np.int32 else np.uint64)


def rolling_bounds(time, starts, ends):
    t = time.numpy()
    lo = np.searchsorted(t, starts.numpy(), side="left").astype(np.int32)
    hi = np.searchsorted(t, ends.numpy(), side="left").astype(np.int32)
    return torch.from_numpy(lo), torch.from_numpy(hi)


def _head_range(keys, perm, j, lo, hi, w0, w1):
    """Windows of [w0, w1) in which position j heads its pair: a..b (k_roll_count / k_roll_fill: head_range)."""
    e = perm[j]
    a = w0 + int(np.searchsorted(hi[w0:w1], e, side="right"))            # first w with hi[w] > e
    b = w0 + int(np.searchsorted(lo[w0:w1], e, side="right")) - 1        # last w with lo[w] <= e
    if j > 0 and keys[j - 1] == keys[j]:
        a = max(a, w0 + int(np.searchsorted(lo[w0:w1], perm[j - 1], side="right")))
    return a, b


def rolling_count(keys, perm, lo, hi, w0, w1, max_run, flags):
    k, p, lo_, hi_ = _unsigned(keys), perm.numpy(), lo.numpy(), hi.numpy()
    m, wn = len(k), w1 - w0
    cnt = np.zeros(m, dtype=np.int32)
    report = np.zeros(wn + 2, dtype=np.int32)
    status = int(flags[0])
    for j in range(m):
        a, b = _head_range(k, p, j, lo_, hi_, w0, w1)
        if b >= a:
            cnt[j] = b - a + 1
            report[a - w0] += 1
            report[b + 1 - w0] -= 1
        if j >= max_run - 1 and k[j] == k[j - (max_run - 1)]:
            status |= LONG_RUN
    report[wn + 1] = status
    return torch.from_numpy(cnt), torch.from_numpy(report)


def rolling_fill(keys, perm, num_nodes, lo, hi, w0, w1, cnt, total, out=None):
    k, p, lo_, hi_, c = _unsigned(keys), perm.numpy(), lo.numpy(), hi.numpy(), cnt.numpy()
    m, wn, bits = len(k), w1 - w0, key_bits(num_nodes)
    ptr = np.concatenate([[0], np.cumsum(c, dtype=np.int64)])
    assert ptr[-1] == total
    wkey, pos = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64)
    for j in range(m):                                                   # k_roll_fill: pair-major {w, j}
        a, b = _head_range(k, p, j, lo_, hi_, w0, w1)
        assert max(b - a + 1, 0) == c[j]
        for w in range(a, b + 1):
            wkey[ptr[j] + w - a], pos[ptr[j] + w - a] = w - w0, j
    order = np.argsort(wkey, kind="stable")                              # the stable sort on the bits of w
    wkey, pos = wkey[order], pos[order]
    if out is None:
        index, weight, offset = torch.empty((2, total), dtype=torch.int64), torch.empty(total, dtype=torch.float32), 0
    else:
        index, weight, offset = out
    nn = np.zeros(wn, dtype=np.uint32)                                   # unsigned, as in the kernel: node 2^31 - 1 makes 2^31
    for q in range(total):                                               # k_roll_emit
        j, w = pos[q], wkey[q]
        key, end = int(k[j]), hi_[w0 + w]
        stop = j
        while stop < m and k[stop] == k[j] and p[stop] < end:            # (the kernel gallops and bisects: perm ascends inside a run)
            stop += 1
        u, v = key >> bits, key & ((1 << bits) - 1)
        index[0, offset + q], index[1, offset + q], weight[offset + q] = int(u), int(v), float(stop - j)
        nn[w] = max(int(nn[w]), max(u, v) + 1)
    return index[:, offset:offset + total], weight[offset:offset + total], torch.from_numpy(nn.view(np.int32))       # (the wrapper's int32 tensor)


def install(monkeypatch):
    """Lets the package's host code run the restatement in place of the kernels, on host tensors."""
    from pathpyg_amd import _hip
    from pathpyg_amd.algorithms import rolling_time_window as rtw
    for fn in (rolling_group, rolling_bounds, rolling_count, rolling_fill):
        monkeypatch.setattr(_hip, fn.__name__, fn)
    monkeypatch.setattr(rtw, "_on_device", lambda edge_index, time: True)


def brute_force(edge_index, time, window):
    """``(edge_index [2, E], edge_weight [E] float32, num_nodes)`` of the window: the events with start <= t < end, merged by node pair."""
    ei, t = np.asarray(edge_index), np.asarray(time)
    keep = (t >= window[0]) & (t < window[1])
    sel = ei[:, keep]
    if sel.shape[1] == 0:
        return np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.float32), 0
    pairs, counts = np.unique(sel.T, axis=0, return_counts=True)
    return pairs.T.astype(np.int64), counts.astype(np.float32), int(sel.max()) + 1


def random_stream(rng, m, n, span, floats=False):
    """A time-sorted stream with ties: ``(edge_index [2, m] int64, time [m])``."""
    ei = rng.integers(0, n, (2, m)).astype(np.int64)
    t = np.sort(rng.integers(0, span, m)).astype(np.int64)
    if floats:
        t = t.astype(np.float64) / 4.0
    return ei, t
