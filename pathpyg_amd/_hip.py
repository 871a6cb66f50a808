"""Device-tensor level wrappers over the C ABI (include/pathpyg_amd.h).

Every function here takes tensors that already live on an MI355X (``tensor.is_cuda``), allocates
outputs and workspaces through PyTorch's caching allocator, launches on the current stream and
returns new tensors on the same device.  PyTorch is only plumbing (memory, streams); all arithmetic
happens in the HIP kernels.  There is no CPU implementation behind these calls.
"""
from __future__ import annotations

import contextlib
import ctypes
import sys
import threading
from typing import NamedTuple

import torch

from ._lib import HipError, check, lib

_DTYPE_CODE = {torch.int32: 0, torch.int64: 1, torch.float32: 2, torch.float64: 3}
_EDGE_AGGR = {"src": 0, "dst": 1, "max": 2, "mul": 3, "add": 4}
_REDUCE = {"sum": 0, "add": 0, "mean": 1, "min": 2, "max": 3}
DELTA_I64, DELTA_F32, DELTA_F64 = 0, 1, 2


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """hipStream_t of the current device's current stream (the raw handle: ~0.4 us instead of the ~2.7 us of building a Stream object —
    a fifth of a shim call's host time, which is what small graphs and the per-rank step of a partitioned run are bound by)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def launch_share(per_mille: int):
    """Persistent launches inside the block take ``per_mille`` / 1000 of the resident workgroup slots (pp_set_launch_share; never fewer
    than 8 workgroups); the previous share comes back on exit.  The share belongs to the CALLING THREAD: autograd runs backward on a
    thread of its own, which keeps its own share, so only the wrappers called directly inside the block are affected."""
    before = lib().pp_set_launch_share(int(per_mille))
    try:
        yield
    finally:
        lib().pp_set_launch_share(before)


def last_persistent_grid() -> int:
    """Workgroups of the calling thread's most recent persistent launch (the kernels whose grid :func:`launch_share` shrinks)."""
    return int(lib().pp_last_persistent_grid())


def _p(t: torch.Tensor | None):
    return None if t is None else t.data_ptr()


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _result(ws: torch.Tensor) -> tuple[int, int]:
    """{size, status} that *_count left at the start of its workspace (one 16-byte D2H copy)."""
    size, status = ws[:16].view(torch.int64).tolist()
    return size, status


def require_device(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("pathpyg_amd kernels need tensors on an MI355X device (got a CPU tensor); there is no CPU path")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} and {t.device}")
        dev = t.device
    return dev


def _edge_index(edge_index: torch.Tensor) -> torch.Tensor:
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"edge_index must have shape [2, E], got {tuple(edge_index.shape)}")
    ei = torch.as_tensor(edge_index)
    if type(ei) is not torch.Tensor:          # tensor subclasses (e.g. an EdgeIndex) -> plain view
        ei = ei.as_subclass(torch.Tensor)
    if ei.dtype != torch.int64:
        ei = ei.to(torch.int64)
    return ei.contiguous()


def _bad_index(status: int, what: str, error=IndexError) -> None:
    if status & 1:
        raise error(f"{what}: node index out of range")


# ------------------------------------------------------------------ primitives
def minmax(a: torch.Tensor) -> tuple[int, int]:
    a = a.contiguous()
    dev = require_device(a)
    with torch.cuda.device(dev):
        out = torch.empty(2, dtype=torch.int64, device=dev)
        check(lib().pp_minmax_i64(_p(a), a.numel(), _p(out), _stream()), "pp_minmax_i64")
        lo, hi = out.tolist()
    return lo, hi


def degree(index: torch.Tensor, num_bins: int) -> torch.Tensor:
    index = index.contiguous()
    dev = require_device(index)
    with torch.cuda.device(dev):
        bins = torch.empty(num_bins, dtype=torch.int32, device=dev)
        check(lib().pp_degree_i64(_p(index), index.numel(), num_bins, _p(bins), _stream()), "pp_degree_i64")
    return bins


def exclusive_scan(values: torch.Tensor) -> torch.Tensor:
    """[0, v0, v0+v1, ..., total] as int64 (PyG ``cumsum``)."""
    values = values.contiguous()
    dev = require_device(values)
    n = values.numel()
    with torch.cuda.device(dev):
        out = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws = _workspace(lib().pp_scan_ws_bytes(n), dev)
        if values.dtype == torch.int32:
            fn, name = lib().pp_exclusive_scan_i32, "pp_exclusive_scan_i32"
        elif values.dtype == torch.int64:
            fn, name = lib().pp_exclusive_scan_i64, "pp_exclusive_scan_i64"
        else:
            raise TypeError("exclusive_scan: int32 or int64 input")
        check(fn(_p(values), n, _p(out), _p(ws), ws.numel(), _stream()), name)
    return out


def sort_pairs(keys: torch.Tensor, values: torch.Tensor | None, begin_bit: int, end_bit: int):
    """Stable radix sort of (key, value) pairs; keys int32/int64 holding NON-NEGATIVE values."""
    keys = keys.contiguous()
    dev = require_device(keys, values)
    n = keys.numel()
    with torch.cuda.device(dev):
        keys_out = torch.empty_like(keys)
        vals_out = torch.empty(n, dtype=torch.int32, device=dev)
        if keys.dtype == torch.int32:
            fn, name, kb = lib().pp_sort_pairs_u32, "pp_sort_pairs_u32", 4
        elif keys.dtype == torch.int64:
            fn, name, kb = lib().pp_sort_pairs_u64, "pp_sort_pairs_u64", 8
        else:
            raise TypeError("sort_pairs: int32 or int64 keys")
        if values is not None:
            values = values.contiguous()
            if values.dtype != torch.int32:
                raise TypeError("sort_pairs: int32 values")
        ws = _workspace(lib().pp_sort_ws_bytes(n, kb), dev)
        check(fn(_p(keys), _p(values), _p(keys_out), _p(vals_out), n, begin_bit, end_bit, _p(ws), ws.numel(), _stream()), name)
    return keys_out, vals_out


# ------------------------------------------------------------------ lifts
def resolve_delta(time_dtype: torch.dtype, delta) -> tuple[int, int, float]:
    """(kind, delta_i, delta_f) describing ``torch.tensor(delta)`` the way the reference's
    ``lift_order_temporal`` sees it (src/pathpyG/algorithms/temporal.py:30,43)."""
    d = delta.detach().cpu() if isinstance(delta, torch.Tensor) else torch.tensor(delta)
    if d.dim() != 0:
        raise ValueError("delta must be a scalar")
    if time_dtype == torch.float64:
        return DELTA_F64, 0, float(d)                  # int / float32 / float64 delta all widen to float64
    if d.dtype.is_floating_point:
        if d.dtype == torch.float64:
            return DELTA_F64, 0, float(d)
        return DELTA_F32, 0, float(d.to(torch.float32))  # python float -> float32 tensor in the reference
    return DELTA_I64, int(d), 0.0


def _drive(gen):
    """Runs a count -> read-back -> fill generator on its own: the generator yields its workspace after the count launch and is sent
    ``(size, status)``."""
    ws = next(gen)
    try:
        gen.send(_result(ws))
    except StopIteration as done:
        return done.value
    raise RuntimeError("count/fill generator yielded twice")


def run_together(*gens):
    """Launches the COUNT phases of several independent count -> fill operations back to back, reads all their {size, status} pairs with
    ONE device-to-host copy (instead of one synchronising read-back each), then runs the fills.  Returns the results in order."""
    try:
        workspaces = [next(g) for g in gens]
        if len({ws.device for ws in workspaces}) > 1:
            raise RuntimeError("run_together: the operations live on different devices")
        if len(workspaces) == 1:
            heads = [_result(workspaces[0])]
        else:
            flat = torch.cat([ws[:16] for ws in workspaces]).view(torch.int64).tolist()
            heads = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(workspaces))]
        results = []
        for g, head in zip(gens, heads):
            try:
                g.send(head)
            except StopIteration as done:
                results.append(done.value)
            else:
                raise RuntimeError("count/fill generator yielded twice")
        return results
    finally:
        for g in gens:          # an error in one operation must not leave the others suspended
            g.close()


def _event_stream(ei: torch.Tensor, time: torch.Tensor, weight: torch.Tensor | None = None):
    """``(time, weight)`` of the events ``ei`` [2, m] as the temporal kernels take them: timestamps int64 or float64 (narrower integers widened),
    contiguous, one per event; ``weight`` None or a contiguous float32 vector of m entries.  ``None``: a weight the builders do not take (the
    caller hands the stream back).  The device is not looked at: every caller runs ``require_device`` first."""
    if time.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8):
        time = time.to(torch.int64)
    if time.dtype not in (torch.int64, torch.float64):
        raise TypeError(f"timestamps must be int64 or float64, got {time.dtype}")
    time = time.contiguous()
    m = ei.size(1)
    if time.numel() != m:
        raise ValueError("time and edge_index disagree on the number of events")
    if weight is not None:
        if weight.dtype != torch.float32 or weight.numel() != m:
            return None
        weight = weight.contiguous()
    return time, weight


def temporal_lift(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int, delta, n_own: int | None = None,
                  id_offset: int = 0) -> torch.Tensor:
    """Second-order event graph of a TIME-SORTED event list: all (i, j) with head(i) == tail(j) and
    t_i < t_j <= t_i + delta, lexicographic, int64 [2, E2].  ``n_own`` / ``id_offset``: edge-range shard —
    only the first ``n_own`` events are sources and ``id_offset`` is added to every id of the result."""
    return _drive(temporal_lift_steps(edge_index, time, num_nodes, delta, n_own, id_offset))


def temporal_lift_steps(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int, delta, n_own: int | None = None, id_offset: int = 0):
    """:func:`temporal_lift` as a count -> fill generator for :func:`run_together`."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, time)
    time, _ = _event_stream(ei, time)
    m = ei.size(1)
    kind, di, df = resolve_delta(time.dtype, delta)
    L = lib()
    # (the device guard is NOT held across the yield: interleaved generators would exit their guards out of order)
    with torch.cuda.device(dev):
        ws = _workspace(L.pp_temporal_ws_bytes(m, num_nodes), dev)
        check(L.pp_temporal_count(_p(ei), _p(time), _DTYPE_CODE[time.dtype], m, m if n_own is None else int(n_own), num_nodes, kind, di, df,
                                  _p(ws), ws.numel(), _stream()), "pp_temporal_count")
    total, status = yield ws
    _bad_index(status, "lift_order_temporal")
    if status & 2:
        raise ValueError("lift_order_temporal: the events are not sorted by time (TemporalGraph sorts them on construction; "
                         "data.time / data.edge_index were modified afterwards)")
    with torch.cuda.device(dev):
        out = torch.empty((2, total), dtype=torch.int64, device=dev)
        check(L.pp_temporal_fill(m, num_nodes, total, int(id_offset), _p(out), _p(ws), ws.numel(), _stream()), "pp_temporal_fill")
    return out


def linegraph_lift(edge_index: torch.Tensor, num_nodes: int, edge_range: tuple[int, int] | None = None) -> torch.Tensor:
    """Line-graph lift of a source-sorted edge list; ``edge_range = (lo, hi)``: edge-range shard — only the edges ``lo .. hi-1`` are
    sources (the block of the global result that starts at the first pair of edge ``lo``), ids stay global."""
    ei = _edge_index(edge_index)
    dev = require_device(ei)
    e = ei.size(1)
    lo, hi = (0, e) if edge_range is None else edge_range
    L = lib()
    with torch.cuda.device(dev):
        ws = _workspace(L.pp_linegraph_ws_bytes(e, num_nodes), dev)
        check(L.pp_linegraph_count(_p(ei), e, lo, hi, num_nodes, _p(ws), ws.numel(), _stream()), "pp_linegraph_count")
        total, status = _result(ws)
        _bad_index(status, "lift_order_edge_index")
        out = torch.empty((2, total), dtype=torch.int64, device=dev)
        check(L.pp_linegraph_fill(e, num_nodes, total, _p(out), _p(ws), ws.numel(), _stream()), "pp_linegraph_fill")
    return out


def edge_attr(edge_index: torch.Tensor, attr: torch.Tensor, aggr: str) -> torch.Tensor:
    if aggr not in _EDGE_AGGR:
        raise ValueError(f"Unknown aggregation method {aggr}")
    ei = _edge_index(edge_index)
    dev = require_device(ei, attr)
    if attr.dtype not in _DTYPE_CODE:
        raise TypeError(f"aggregate_node_attributes: unsupported attribute dtype {attr.dtype}")
    attr = attr.contiguous()
    n = attr.size(0)
    width = attr.numel() // n if n else 1
    e = ei.size(1)
    with torch.cuda.device(dev):
        out = torch.empty((e,) + tuple(attr.shape[1:]), dtype=attr.dtype, device=dev)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib().pp_edge_attr(_p(ei), e, _p(attr), _DTYPE_CODE[attr.dtype], n, max(width, 1), _EDGE_AGGR[aggr], _p(out), _p(status),
                                 _stream()), "pp_edge_attr")
        _bad_index(int(status.item()), "aggregate_node_attributes")
    return out


def extend_node_sequence(edge_index: torch.Tensor, node_sequence: torch.Tensor) -> torch.Tensor:
    ei = _edge_index(edge_index)
    dev = require_device(ei, node_sequence)
    ns = node_sequence.to(torch.int64).contiguous()
    n_rows, k = ns.shape
    e = ei.size(1)
    with torch.cuda.device(dev):
        out = torch.empty((e, k + 1), dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib().pp_extend_node_sequence(_p(ei), e, _p(ns), n_rows, k, _p(out), _p(status), _stream()), "pp_extend_node_sequence")
        _bad_index(int(status.item()), "node sequence extension")
    return out


def gather_concat(rows: torch.Tensor, idx: torch.Tensor, suffix: torch.Tensor) -> torch.Tensor:
    """``cat([rows[idx], suffix[:, None]], 1)`` for int64 ``rows [R, k]`` -> ``[n, k+1]``."""
    dev = require_device(rows, idx, suffix)
    rows = rows.to(torch.int64).contiguous()
    idx = idx.to(torch.int64).contiguous()
    suffix = suffix.to(torch.int64).contiguous()
    n, k = idx.numel(), rows.size(1)
    with torch.cuda.device(dev):
        out = torch.empty((n, k + 1), dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib().pp_gather_concat(_p(rows), rows.size(0), k, _p(idx), _p(suffix), n, _p(out), _p(status), _stream()), "pp_gather_concat")
        _bad_index(int(status.item()), "node sequence gather")
    return out


# ------------------------------------------------------------------ aggregation
def unique_rows(rows: torch.Tensor, value_range: tuple[int, int] | None = None):
    """``torch.unique(rows, dim=0, return_inverse=True)`` for int64 ``[M, k]`` rows."""
    dev = require_device(rows)
    rows = rows.to(torch.int64).contiguous()
    m, k = rows.shape
    L = lib()
    with torch.cuda.device(dev):
        inverse = torch.empty(m, dtype=torch.int64, device=dev)
        if m == 0:
            return rows.new_empty((0, k)), inverse
        lo, hi = value_range if value_range is not None else minmax(rows)
        ws = _workspace(L.pp_unique_rows_ws_bytes(m), dev)
        check(L.pp_unique_rows_count(_p(rows), m, k, lo, hi, _p(inverse), _p(ws), ws.numel(), _stream()), "pp_unique_rows_count")
        n_unique, _ = _result(ws)
        uniq = torch.empty((n_unique, k), dtype=torch.int64, device=dev)
        check(L.pp_unique_rows_fill(_p(rows), m, k, n_unique, _p(uniq), _p(ws), ws.numel(), _stream()), "pp_unique_rows_fill")
    return uniq, inverse


UNIT = "unit"           # `weight=UNIT`: every instance edge weighs 1.0 (the reference's default torch.ones) without materialising the vector


def coalesce(edge_index: torch.Tensor, weight, num_nodes: int, reduce: str = "sum",
             remap: torch.Tensor | None = None, want_inverse: bool = False, col_block: tuple | None = None):
    """PyG ``coalesce`` of ``remap[edge_index]`` (or ``edge_index``): (row, col)-sorted distinct edges + reduced weights.
    ``weight``: a vector, ``None`` (no weights) or :data:`UNIT` (float32 ones: the merged weight is the run length, no gather).
    ``want_inverse`` additionally returns, per input edge, the index of the merged edge it went into.
    ``col_block = (col_base [num_nodes] int64, col_bits)``: every column of row r lies in ``[col_base[r], col_base[r] + 2**col_bits)``
    (De Bruijn layers): shorter sort keys, same result."""
    return _drive(coalesce_steps(edge_index, weight, num_nodes, reduce, remap, want_inverse, col_block))


def coalesce_steps(edge_index: torch.Tensor, weight, num_nodes: int, reduce: str = "sum",
                   remap: torch.Tensor | None = None, want_inverse: bool = False, col_block: tuple | None = None):
    """:func:`coalesce` as a count -> fill generator for :func:`run_together`."""
    if reduce not in _REDUCE:
        raise ValueError(f"unknown reduce {reduce}")
    ei = _edge_index(edge_index)
    unit = isinstance(weight, str)
    if unit:
        if weight != UNIT:
            raise ValueError(f"edge weights must be a tensor, None or the marker {UNIT!r}, got {weight!r}")
        weight = None
    dev = require_device(ei, weight, remap)
    e = ei.size(1)
    if weight is not None:
        if weight.dtype not in _DTYPE_CODE:
            raise TypeError(f"edge weights of dtype {weight.dtype} are not supported")
        if weight.dim() != 1 or weight.numel() != e:
            raise ValueError("edge_weight must be a vector with one entry per edge")
        weight = weight.contiguous()
    if remap is not None:
        remap = remap.to(torch.int64).contiguous()
    col_base, col_bits = (None, 0) if col_block is None else (col_block[0].to(torch.int64).contiguous(), int(col_block[1]))
    if col_base is not None and col_base.numel() != num_nodes:
        raise ValueError("col_base must hold one entry per node")
    if e >= 0x7fffffff:          # (pp_coalesce_count's refusal, before a workspace of ~40 bytes per edge is allocated for it)
        raise HipError(f"pp_coalesce_count: more than 2^31 edges ({e})")
    L = lib()
    with torch.cuda.device(dev):
        ws = _workspace(L.pp_coalesce_ws_bytes(e), dev)
        check(L.pp_coalesce_count(_p(ei), e, _p(remap), 0 if remap is None else remap.numel(), num_nodes, _p(col_base), col_bits,
                                  _p(ws), ws.numel(), _stream()), "pp_coalesce_count")
    n_out, status = yield ws
    # the reference fails in EdgeIndex.validate() with a ValueError when an index exceeds the number of distinct nodes
    # (lift_order.py:133-147: layer-1 quirk, node ids are used as given while num_nodes counts the distinct ones)
    _bad_index(status, "aggregate_edge_index (an edge refers to a node id >= number of distinct nodes)", ValueError)
    with torch.cuda.device(dev):
        out_index = torch.empty((2, n_out), dtype=torch.int64, device=dev)
        out_weight = (torch.empty(n_out, dtype=torch.float32, device=dev) if unit else None) if weight is None else \
            torch.empty(n_out, dtype=weight.dtype, device=dev)
        check(L.pp_coalesce_fill(_p(weight), 2 if weight is None else _DTYPE_CODE[weight.dtype], _REDUCE[reduce], e, n_out, num_nodes,
                                 _p(col_base), col_bits, _p(out_index), _p(out_weight), _p(ws), ws.numel(), _stream()), "pp_coalesce_fill")
        if want_inverse:
            inverse = torch.empty(e, dtype=torch.int64, device=dev)
            check(L.pp_coalesce_inverse(e, _p(inverse), _p(ws), ws.numel(), _stream()), "pp_coalesce_inverse")
            return out_index, out_weight, inverse
    return out_index, out_weight


# ------------------------------------------------------------------ Graph bookkeeping
def _ordered_dtype(a: torch.Tensor) -> torch.Tensor:
    if a.dtype in (torch.int64, torch.float64):
        return a.contiguous()
    if a.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool):
        return a.to(torch.int64).contiguous()
    if a.dtype in (torch.float32, torch.float16, torch.bfloat16):
        return a.to(torch.float64).contiguous()      # exact widening keeps the order
    raise TypeError(f"cannot order values of dtype {a.dtype}")


def is_sorted(a: torch.Tensor) -> bool:
    a = _ordered_dtype(a)
    dev = require_device(a)
    with torch.cuda.device(dev):
        out = torch.empty(1, dtype=torch.int64, device=dev)
        if a.dtype == torch.float64:
            check(lib().pp_count_descents_f64(_p(a), a.numel(), _p(out), _stream()), "pp_count_descents_f64")
        else:
            check(lib().pp_count_descents_i64(_p(a), a.numel(), _p(out), _stream()), "pp_count_descents_i64")
        return int(out.item()) == 0


def time_stats(time: torch.Tensor) -> tuple[int, int, int]:
    """``(descents, min, max)`` of a timestamp vector with ONE read-back (float64: min = max = 0)."""
    time = _ordered_dtype(time)
    dev = require_device(time)
    with torch.cuda.device(dev):
        out = torch.empty(3, dtype=torch.int64, device=dev)
        check(lib().pp_time_stats(_p(time), _DTYPE_CODE[time.dtype], time.numel(), _p(out), _stream()), "pp_time_stats")
        descents, lo, hi = out.tolist()
    return descents, lo, hi


def gather_events(edge_index: torch.Tensor, time: torch.Tensor, perm: torch.Tensor):
    """``(edge_index[:, perm], time[perm])`` in one pass (time int64 or float64)."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, time, perm)
    if time.dtype not in (torch.int64, torch.float64):
        raise TypeError("gather_events: timestamps must be int64 or float64")
    time, perm = time.contiguous(), perm.to(torch.int64).contiguous()
    m = ei.size(1)
    with torch.cuda.device(dev):
        out_ei, out_t = torch.empty_like(ei), torch.empty_like(time)
        status = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib().pp_gather_events(_p(ei), _p(time), _p(perm), m, _p(out_ei), _p(out_t), _p(status), _stream()), "pp_gather_events")
    return out_ei, out_t


def argsort(keys: torch.Tensor, value_range: tuple[int, int] | None = None) -> torch.Tensor:
    """Stable argsort of an integer or floating-point vector -> int64 permutation."""
    keys = _ordered_dtype(keys)
    dev = require_device(keys)
    n = keys.numel()
    with torch.cuda.device(dev):
        perm = torch.empty(n, dtype=torch.int64, device=dev)
        if n == 0:
            return perm
        if keys.dtype == torch.float64:
            ws = _workspace(lib().pp_argsort_ws_bytes(n), dev)
            check(lib().pp_argsort_f64(_p(keys), n, _p(perm), _p(ws), ws.numel(), _stream()), "pp_argsort_f64")
            return perm
        lo, hi = value_range if value_range is not None else minmax(keys)
        ws = _workspace(lib().pp_argsort_ws_bytes(n), dev)
        check(lib().pp_argsort_i64(_p(keys), n, lo, hi, _p(perm), _p(ws), ws.numel(), _stream()), "pp_argsort_i64")
    return perm


# ------------------------------------------------------------------ ingest (csrc/pp_ingest.hip)
INGEST_MAX_CHUNK = 0x7fffffff - 1       # pp_ingest_*: line offsets are int32


def ingest_workspace(n_bytes: int, device) -> torch.Tensor:
    """The workspace one :func:`ingest_index` / :func:`ingest_parse` pair shares."""
    return _workspace(lib().pp_ingest_index_ws_bytes(int(n_bytes)), device)


def ingest_index(chunk: torch.Tensor, sep: int, ws: torch.Tensor) -> torch.Tensor:
    """Offsets (int32, file order) of the first byte of every non-blank line of ``chunk`` (uint8, on the device).  The vector has the
    capacity no qualifying chunk exceeds; the line count stays on the device (in ``ws``) for :func:`ingest_parse`."""
    dev = require_device(chunk, ws)
    chunk = chunk.contiguous()
    n = chunk.numel()
    with torch.cuda.device(dev):
        line_start = torch.empty((n + 1) // 6 + 1, dtype=torch.int32, device=dev)
        check(lib().pp_ingest_index(_p(chunk), n, int(sep), _p(line_start), line_start.numel(), _p(ws), ws.numel(), _stream()), "pp_ingest_index")
    return line_start


def ingest_parse(chunk: torch.Tensor, sep: int, line_start: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """``[3, capacity]`` int64: rows ``v``, ``w``, ``t``; column ``i`` is line ``i`` of :func:`ingest_index`.  Only the first
    ``n_lines`` columns (:func:`ingest_result`) are written, and they mean something only when the status is 0."""
    dev = require_device(chunk, line_start, ws)
    chunk = chunk.contiguous()
    cap = line_start.numel()
    with torch.cuda.device(dev):
        cols = torch.empty((3, cap), dtype=torch.int64, device=dev)
        check(lib().pp_ingest_parse(_p(chunk), chunk.numel(), int(sep), _p(line_start), cap, _p(cols[0]), _p(cols[1]), _p(cols[2]),
                                    _p(ws), ws.numel(), _stream()), "pp_ingest_parse")
    return cols


def ingest_result(ws: torch.Tensor) -> tuple[int, int, int]:
    """``(n_lines, status, smallest offending byte offset)`` of a chunk: the one read-back of its index + parse."""
    n_lines, status, bad_at, _ = ws[:32].view(torch.int64).tolist()
    return n_lines, status, bad_at


class TokenIndex(NamedTuple):
    """What :func:`ingest_tokens_index` leaves on the device for :func:`ingest_tokens_parse` (capacities, not counts)."""
    token_start: torch.Tensor           # [cap] int32
    token_line: torch.Tensor            # [cap] int32
    line_first_token: torch.Tensor      # [cap + 1] int32


def ingest_tokens_workspace(n_bytes: int, device) -> torch.Tensor:
    """The workspace one :func:`ingest_tokens_index` / :func:`ingest_tokens_parse` pair shares."""
    return _workspace(lib().pp_ingest_tokens_ws_bytes(int(n_bytes)), device)


def ingest_tokens_index(chunk: torch.Tensor, sep: int, ws: torch.Tensor) -> TokenIndex:
    """Token index of an n-gram ``chunk`` (uint8, on the device): offset and line of every token, first token of every non-blank line,
    all in file order.  The vectors have the capacity no qualifying chunk exceeds (``n // 2 + 1`` tokens and lines); both counts stay on
    the device (in ``ws``) for :func:`ingest_tokens_parse`."""
    dev = require_device(chunk, ws)
    chunk = chunk.contiguous()
    n = chunk.numel()
    cap = n // 2 + 1
    with torch.cuda.device(dev):
        index = TokenIndex(torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                           torch.empty(cap + 1, dtype=torch.int32, device=dev))
        check(lib().pp_ingest_tokens_index(_p(chunk), n, int(sep), _p(index.token_start), _p(index.token_line), cap,
                                           _p(index.line_first_token), cap, _p(ws), ws.numel(), _stream()), "pp_ingest_tokens_index")
    return index


def ingest_tokens_parse(chunk: torch.Tensor, sep: int, weight: bool, index: TokenIndex, ws: torch.Tensor):
    """``(nodes int64, lengths int64, weights float32 | None)`` at the capacity of ``index``: the node IDs of all walks in file order, the
    nodes per walk, and (``weight``) the last token of every line.  Only the first ``n_tokens - n_lines`` (``weight``) or ``n_tokens``
    nodes and the first ``n_lines`` lengths and weights (:func:`ingest_tokens_result`) are written, and they mean something only when the
    status is 0."""
    dev = require_device(chunk, ws, *index)
    chunk = chunk.contiguous()
    cap = index.token_start.numel()
    with torch.cuda.device(dev):
        nodes = torch.empty(cap, dtype=torch.int64, device=dev)
        lengths = torch.empty(cap, dtype=torch.int64, device=dev)
        weights = torch.empty(cap, dtype=torch.float32, device=dev) if weight else None
        check(lib().pp_ingest_tokens_parse(_p(chunk), chunk.numel(), int(sep), 1 if weight else 0, _p(index.token_start), _p(index.token_line), cap,
                                           _p(index.line_first_token), cap, _p(nodes), _p(lengths), _p(weights), _p(ws), ws.numel(), _stream()),
              "pp_ingest_tokens_parse")
    return nodes, lengths, weights


def ingest_tokens_result(ws: torch.Tensor) -> tuple[int, int, int, int]:
    """``(n_lines, n_tokens, status, smallest offending byte offset)`` of a chunk: the one read-back of its index + parse."""
    n_lines, status, bad_at, n_tokens = ws[:32].view(torch.int64).tolist()
    return n_lines, n_tokens, status, bad_at


def ptr_from_sorted(sorted_index: torch.Tensor, num_rows: int) -> torch.Tensor:
    sorted_index = sorted_index.to(torch.int64).contiguous()
    dev = require_device(sorted_index)
    with torch.cuda.device(dev):
        ptr = torch.empty(num_rows + 1, dtype=torch.int64, device=dev)
        check(lib().pp_ptr_from_sorted_i64(_p(sorted_index), sorted_index.numel(), num_rows, _p(ptr), _stream()), "pp_ptr_from_sorted_i64")
    return ptr


def temporal_bfs(edge_index: torch.Tensor, num_nodes: int, event_graph: torch.Tensor):
    """All-pairs shortest time-respecting paths over a lifted event graph (``event_graph`` = ``temporal_lift`` output of the same
    time-sorted ``edge_index``): ``(dist int32 [n,n] with -1 = unreachable, pred int64 [n,n])``."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, event_graph)
    m, n = ei.size(1), int(num_nodes)
    succ_ptr = ptr_from_sorted(event_graph[0], m)
    succ = event_graph[1].contiguous()
    by_src = argsort(ei[0], (0, max(n - 1, 0)))
    by_src_ptr = ptr_from_sorted(ei[0][by_src], n)
    L = lib()
    with torch.cuda.device(dev):
        dist = torch.empty((n, n), dtype=torch.int32, device=dev)
        pred = torch.empty((n, n), dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_temporal_bfs_ws_bytes(m, n), dev)
        check(L.pp_temporal_bfs(_p(ei), m, n, _p(succ_ptr), _p(succ), _p(by_src_ptr), _p(by_src), _p(dist), _p(pred), _p(ws), ws.numel(),
                                _stream()), "pp_temporal_bfs")
    return dist, pred


def temporal_betweenness(edge_index: torch.Tensor, num_nodes: int, event_graph: torch.Tensor) -> torch.Tensor:
    """Temporal betweenness per node index (float64 [n]) over a lifted event graph of the time-sorted ``edge_index``."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, event_graph)
    m, n = ei.size(1), int(num_nodes)
    succ_ptr = ptr_from_sorted(event_graph[0], m)
    succ = event_graph[1].contiguous()
    by_src = argsort(ei[0], (0, max(n - 1, 0)))
    by_src_ptr = ptr_from_sorted(ei[0][by_src], n)
    by_dst = argsort(ei[1], (0, max(n - 1, 0)))
    by_dst_ptr = ptr_from_sorted(ei[1][by_dst], n)
    L = lib()
    with torch.cuda.device(dev):
        parts = int(L.pp_temporal_betweenness_parts(m, n))
        partial = torch.zeros((parts, n), dtype=torch.float64, device=dev)
        ws = _workspace(L.pp_temporal_betweenness_ws_bytes(m, n), dev)
        check(L.pp_temporal_betweenness(_p(ei), m, n, _p(succ_ptr), _p(succ), _p(by_src_ptr), _p(by_src), _p(by_dst_ptr), _p(by_dst),
                                        _p(partial), _p(ws), ws.numel(), _stream()), "pp_temporal_betweenness")
        return partial.sum(dim=0)


# ------------------------------------------------------------------ static shortest paths (pp_graph_paths.hip)
def _graph_csr(row_ptr: torch.Tensor, col: torch.Tensor, num_nodes: int, sources: torch.Tensor):
    row_ptr, col, sources = (t.to(torch.int64).contiguous() for t in (row_ptr, col, sources))
    dev = require_device(row_ptr, col, sources)
    n, m = int(num_nodes), col.numel()
    if row_ptr.numel() != n + 1:
        raise ValueError(f"row_ptr must have num_nodes + 1 = {n + 1} entries, got {row_ptr.numel()}")
    if sources.numel():
        lo, hi = minmax(sources)
        if lo < 0 or hi >= n:
            raise IndexError(f"source node index out of range [0, {n})")
    return row_ptr, col, sources, dev, n, m


def graph_bfs_dense(row_ptr: torch.Tensor, col: torch.Tensor, num_nodes: int, sources: torch.Tensor):
    """Unit-weight shortest paths from every entry of ``sources`` on a source-major CSR: ``(dist, pred)``, both int32
    ``[len(sources), n]``; ``dist`` -1 = unreachable, ``pred`` the largest tight predecessor index, -9999 where there is none.
    The only caller of ``pp_graph_bfs`` that allocates anything of size sources x n."""
    row_ptr, col, sources, dev, n, m = _graph_csr(row_ptr, col, num_nodes, sources)
    k = sources.numel()
    L = lib()
    with torch.cuda.device(dev):
        dist = torch.empty((k, n), dtype=torch.int32, device=dev)
        pred = torch.empty((k, n), dtype=torch.int32, device=dev)
        ws = _workspace(L.pp_graph_bfs_ws_bytes(n, k), dev)
        check(L.pp_graph_bfs(_p(row_ptr), _p(col), n, m, _p(sources), k, _p(dist), _p(pred), None, None, None, _p(ws), ws.numel(), _stream()),
              "pp_graph_bfs")
    return dist, pred


def graph_bfs_totals(row_ptr: torch.Tensor, col: torch.Tensor, num_nodes: int, sources: torch.Tensor):
    """The distance totals of the same searches without any per-pair output: ``(reach_in [n], dist_in [n], totals [3])`` int64 —
    per node the number of sources (other than itself) that reach it and the sum of their distances; the sum of all finite
    distances, the largest one and the number of (source, other node) pairs without a path.  O(n) memory per workgroup."""
    row_ptr, col, sources, dev, n, m = _graph_csr(row_ptr, col, num_nodes, sources)
    k = sources.numel()
    L = lib()
    with torch.cuda.device(dev):
        acc = torch.zeros(2 * n + 3, dtype=torch.int64, device=dev)
        reach_in, dist_in, totals = acc[:n], acc[n:2 * n], acc[2 * n:]
        ws = _workspace(L.pp_graph_bfs_ws_bytes(n, k), dev)
        check(L.pp_graph_bfs(_p(row_ptr), _p(col), n, m, _p(sources), k, None, None, _p(reach_in), _p(dist_in), _p(totals), _p(ws), ws.numel(),
                             _stream()), "pp_graph_bfs")
    return reach_in, dist_in, totals


def graph_betweenness(row_ptr: torch.Tensor, col: torch.Tensor, num_nodes: int, sources: torch.Tensor):
    """Betweenness in the reference's form from the given sources: ``(bw float64 [n], reached bool [n], overflow bool [n])``; ``reached``
    marks the nodes some source reached at distance >= 1, ``overflow`` those to which some searched source has 2**1024 or more shortest
    paths — if any is set, ``bw`` is meaningless.  The per-workgroup rows are summed in row order: the same bits on every run while the
    path counts stay below 2**53."""
    row_ptr, col, sources, dev, n, m = _graph_csr(row_ptr, col, num_nodes, sources)
    k = sources.numel()
    L = lib()
    with torch.cuda.device(dev):
        parts = int(L.pp_graph_betweenness_parts(n, k))
        partial = torch.zeros((parts, n), dtype=torch.float64, device=dev)
        reached = torch.zeros(n, dtype=torch.int32, device=dev)
        ws = _workspace(L.pp_graph_betweenness_ws_bytes(n, k), dev)
        check(L.pp_graph_betweenness(_p(row_ptr), _p(col), n, m, _p(sources), k, _p(partial), _p(reached), _p(ws), ws.numel(), _stream()),
              "pp_graph_betweenness")
        return partial.sum(dim=0), (reached & 1) != 0, (reached & 2) != 0


# ------------------------------------------------------------------ connected components (pp_graph_components.hip)
def _graph_both(edge_index: torch.Tensor, num_nodes: int, csr, csc):
    ei = _edge_index(edge_index)
    n, m = int(num_nodes), ei.size(1)
    parts = [None, None, None, None]
    if csr is not None:
        parts = [t.to(torch.int64).contiguous() for t in (*csr, *csc)]
        for ptr, idx, name in ((parts[0], parts[1], "row_ptr / col"), (parts[2], parts[3], "col_ptr / row")):
            if ptr.numel() != n + 1 or idx.numel() != m:
                raise ValueError(f"{name} must have num_nodes + 1 = {n + 1} and {m} entries, got {ptr.numel()} and {idx.numel()}")
    dev = require_device(ei, *parts)
    return ei, parts, dev, n, m


def graph_components(edge_index: torch.Tensor, num_nodes: int, csr=None, csc=None):
    """Connected components of the stored edges: weak from the edge list alone; strong when ``csr = (row_ptr, col)`` and
    ``csc = (col_ptr, row)`` are given.  Returns ``(count int64 [1], labels int32 [n], sizes int64 [n], stats)``, all tensors on the
    device: labels numbered by each component's smallest node index, the first ``count`` entries of ``sizes`` valid; ``stats`` is the
    host list ``[rounds, trim sweeps, colour sweeps, backward sweeps]``."""
    strong = csr is not None
    if strong != (csc is not None):
        raise ValueError("graph_components: the CSR and the CSC come together")
    ei, (row_ptr, col, col_ptr, row), dev, n, m = _graph_both(edge_index, num_nodes, csr, csc)
    L = lib()
    with torch.cuda.device(dev):
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        acc = torch.empty(n + 1, dtype=torch.int64, device=dev)
        sizes, count = acc[:n], acc[n:]
        stats = (ctypes.c_int64 * 4)()
        ws = _workspace(L.pp_graph_components_ws_bytes(n, m, int(strong)), dev)
        check(L.pp_graph_components(_p(ei), m, n, _p(row_ptr), _p(col), _p(col_ptr), _p(row), int(strong), _p(labels), _p(sizes), _p(count),
                                    ctypes.addressof(stats), _p(ws), ws.numel(), _stream()), "pp_graph_components")
    return count, labels, sizes, list(stats)


def graph_components_largest(sizes: torch.Tensor, count: torch.Tensor) -> tuple[int, int]:
    """``(label, size)`` of the largest component, the smallest label among equals (one 16-byte read-back); ``(-1, 0)`` without components."""
    dev = require_device(sizes, count)
    with torch.cuda.device(dev):
        out = torch.empty(2, dtype=torch.int64, device=dev)
        check(lib().pp_graph_components_largest(_p(sizes), _p(count), _p(out), _stream()), "pp_graph_components_largest")
        label, size = out.tolist()
    return label, size


def graph_component_nodes(labels: torch.Tensor, keep: int, size: int) -> torch.Tensor:
    """The ``size`` node indices that carry the label ``keep``, ascending (int64, on the device)."""
    labels = labels.contiguous()
    dev = require_device(labels)
    n = labels.numel()
    L = lib()
    with torch.cuda.device(dev):
        nodes = torch.empty(int(size), dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_graph_component_keep_ws_bytes(n), dev)
        check(L.pp_graph_component_nodes(_p(labels), n, int(keep), _p(nodes), nodes.numel(), _p(count), _p(ws), ws.numel(), _stream()),
              "pp_graph_component_nodes")
    return nodes


def graph_component_edges(edge_index: torch.Tensor, labels: torch.Tensor, keep: int, new_index: torch.Tensor) -> torch.Tensor:
    """The stored edges with both ends labelled ``keep``, in stored order, renumbered through ``new_index`` [n]: int64 ``[2, kept]``."""
    ei = _edge_index(edge_index)
    labels, new_index = labels.contiguous(), new_index.to(torch.int64).contiguous()
    dev = require_device(ei, labels, new_index)
    n, m = labels.numel(), ei.size(1)
    if new_index.numel() != n:
        raise ValueError(f"new_index must have {n} entries, got {new_index.numel()}")
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty((2, m), dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_graph_component_keep_ws_bytes(m), dev)
        check(L.pp_graph_component_edges(_p(ei), m, n, _p(labels), int(keep), _p(new_index), _p(out), _p(count), _p(ws), ws.numel(), _stream()),
              "pp_graph_component_edges")
        kept = int(count.item())
        return out[:, :kept].contiguous()


# ------------------------------------------------------------------ graph statistics (pp_graph_triads.hip)
# Work split of the list intersections, None = the library's choice (include/pathpyg_amd.h): the lanes per pair of lists (a power of two up to
# 64) and the length of the shorter list from which a pair gets a whole workgroup.  They change the time, never an integer result.
TRIAD_GROUP: int | None = None
TRIAD_HEAVY_MIN: int | None = None


def _triad_split() -> tuple[int, int]:
    return int(TRIAD_GROUP or 0), int(TRIAD_HEAVY_MIN or 0)


def count_unordered(edge_index: torch.Tensor) -> int:
    """Number of positions at which the stored edge list is not strictly (row, col)-increasing (one 8-byte read-back)."""
    ei = _edge_index(edge_index)
    dev = require_device(ei)
    with torch.cuda.device(dev):
        out = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib().pp_graph_count_unordered(_p(ei), ei.size(1), _p(out), _stream()), "pp_graph_count_unordered")
        return int(out.item())


def _simple(row_ptr, row, col, num_nodes: int):
    row_ptr, row, col = (t.to(torch.int64).contiguous() for t in (row_ptr, row, col))
    dev = require_device(row_ptr, row, col)
    n, ms = int(num_nodes), col.numel()
    if row_ptr.numel() != n + 1 or row.numel() != ms:
        raise ValueError(f"row_ptr and row must have num_nodes + 1 = {n + 1} and {ms} entries, got {row_ptr.numel()} and {row.numel()}")
    return row_ptr, row, col, dev, n, ms


def graph_triad_entry_counts(row_ptr, row, col, num_nodes: int, e0: int, e1: int) -> torch.Tensor:
    """``cnt[e - e0] = |S(col[e]) ∩ S(row[e])|`` (int64) for the entries ``e0 <= e < e1`` of a simple successor structure."""
    row_ptr, row, col, dev, n, ms = _simple(row_ptr, row, col, num_nodes)
    if not 0 <= e0 <= e1 <= ms:
        raise IndexError(f"entry range [{e0}, {e1}) outside [0, {ms}]")
    group, heavy = _triad_split()
    L = lib()
    with torch.cuda.device(dev):
        cnt = torch.empty(e1 - e0, dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_graph_meet_ws_bytes(e1 - e0), dev)
        check(L.pp_graph_triad_entry_counts(_p(row_ptr), _p(row), _p(col), n, ms, e0, e1, group, heavy, _p(cnt), _p(ws), ws.numel(), _stream()),
              "pp_graph_triad_entry_counts")
    return cnt


def graph_triad_node_counts(row_ptr, row, col, num_nodes: int) -> torch.Tensor:
    """The number of closed triads of every node (int64 ``[n]``) from a simple successor structure."""
    row_ptr, row, col, dev, n, ms = _simple(row_ptr, row, col, num_nodes)
    group, heavy = _triad_split()
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty(n, dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_graph_triad_node_counts_ws_bytes(ms), dev)
        check(L.pp_graph_triad_node_counts(_p(row_ptr), _p(row), _p(col), n, ms, group, heavy, _p(out), _p(ws), ws.numel(), _stream()),
              "pp_graph_triad_node_counts")
    return out


def graph_triad_fill(row_ptr, col, num_nodes: int, v: int, offset: torch.Tensor, total: int) -> torch.Tensor:
    """The closed triads of node ``v`` as int64 ``[2, total]``; ``offset`` = the exclusive scan of its row's entry counts."""
    row_ptr, col, offset = (t.to(torch.int64).contiguous() for t in (row_ptr, col, offset))
    dev = require_device(row_ptr, col, offset)
    n = int(num_nodes)
    if row_ptr.numel() != n + 1:
        raise ValueError(f"row_ptr must have num_nodes + 1 = {n + 1} entries, got {row_ptr.numel()}")
    if not 0 <= v < n:
        raise IndexError(f"node index out of range [0, {n})")
    with torch.cuda.device(dev):
        out = torch.empty((2, int(total)), dtype=torch.int64, device=dev)
        check(lib().pp_graph_triad_fill(_p(row_ptr), _p(col), n, col.numel(), int(v), _p(offset), offset.numel(), int(total), _p(out), _stream()),
              "pp_graph_triad_fill")
    return out


PAIR_MEASURES = {"overlap": 1, "jaccard": 2, "adamic_adar": 3, "cosine": 4}


def pair_measure(measure: str, n: int, pairs, common, dot=None, aa=None, sizes=None, norm2=None, indeg=None) -> torch.Tensor:
    """float64 ``[P]``: one similarity measure per pair from the integers of :func:`graph_pair_meets` (``pp_pair_measure``)."""
    dev = require_device(pairs, common, dot, aa, sizes, norm2, indeg)
    P = common.numel()
    with torch.cuda.device(dev):
        out = torch.empty(P, dtype=torch.float64, device=dev)
        check(lib().pp_pair_measure(PAIR_MEASURES[measure], _p(common), _p(dot), _p(aa), _p(sizes), _p(norm2), _p(indeg), _p(pairs), P, int(n),
                                    _p(out), _stream()), "pp_pair_measure")
    return out


def graph_pair_meets(row_ptr, col, mult, num_nodes: int, pairs: torch.Tensor, deg_ptr=None, table=None, want_dot: bool = False,
                     want_sizes: bool = False):
    """``(common int64 [P], dot int64 [P] | None, aa float64 [P] | None, sizes int64 [2, P] | None)`` for the node index pairs ``pairs`` [2, P] on a simple successor
    structure; ``aa`` when ``table`` (float64, by stored out-degree) and ``deg_ptr`` (the stored row pointers) are given."""
    row_ptr, col = row_ptr.to(torch.int64).contiguous(), col.to(torch.int64).contiguous()
    pairs = _edge_index(pairs)
    mult = None if mult is None else mult.to(torch.int64).contiguous()
    dev = require_device(row_ptr, col, mult, pairs, deg_ptr, table)
    n, ms, P = int(num_nodes), col.numel(), pairs.size(1)
    if row_ptr.numel() != n + 1 or (mult is not None and mult.numel() != ms):
        raise ValueError("row_ptr must have num_nodes + 1 entries and mult one per entry of col")
    if P:
        lo, hi = minmax(pairs)
        if lo < 0 or hi >= n:
            raise IndexError(f"node index out of range [0, {n})")
    if table is not None:
        table, deg_ptr = table.to(torch.float64).contiguous(), deg_ptr.to(torch.int64).contiguous()
        if deg_ptr.numel() != n + 1 or table.numel() < 1:
            raise ValueError("deg_ptr must have num_nodes + 1 entries and the table at least one")
    group, heavy = _triad_split()
    L = lib()
    with torch.cuda.device(dev):
        common = torch.empty(P, dtype=torch.int64, device=dev)
        dot = torch.empty(P, dtype=torch.int64, device=dev) if want_dot else None
        aa = torch.empty(P, dtype=torch.float64, device=dev) if table is not None else None
        sizes = torch.empty((2, P), dtype=torch.int64, device=dev) if want_sizes else None
        ws = _workspace(L.pp_graph_meet_ws_bytes(P), dev)
        check(L.pp_graph_pair_meets(_p(row_ptr), _p(col), _p(mult), n, ms, _p(pairs), P, _p(deg_ptr), _p(table), 0 if table is None else table.numel(),
                                    group, heavy, _p(common), _p(dot), _p(aa), _p(sizes), _p(ws), ws.numel(), _stream()), "pp_graph_pair_meets")
    return common, dot, aa, sizes


def degree_product_sum(edge_index: torch.Tensor, num_nodes: int, a: torch.Tensor | None, b: torch.Tensor) -> int:
    """The exact integer ``sum over stored edges of a[src] * b[dst]`` (``a = None``: of ``b[dst]``); ``a``, ``b`` int32 ``[n]``."""
    ei = _edge_index(edge_index)
    a = None if a is None else a.to(torch.int32).contiguous()
    b = b.to(torch.int32).contiguous()
    dev = require_device(ei, a, b)
    n = int(num_nodes)
    if b.numel() != n or (a is not None and a.numel() != n):
        raise ValueError(f"degree vectors must have num_nodes = {n} entries")
    with torch.cuda.device(dev):
        out = torch.empty(1, dtype=torch.int64, device=dev)
        check(lib().pp_degree_product_sum(_p(ei), ei.size(1), n, _p(a), _p(b), _p(out), _stream()), "pp_degree_product_sum")
        return int(out.item())


def graph_clustering(triads: torch.Tensor, deg: torch.Tensor, want_coeff: bool = True, want_mean: bool = False):
    """``(coeff float64 [n] | None, mean float64 [1] | None)`` from the closed-triad counts (int64) and the degrees (int32) of all nodes."""
    triads, deg = triads.to(torch.int64).contiguous(), deg.to(torch.int32).contiguous()
    dev = require_device(triads, deg)
    n = triads.numel()
    if deg.numel() != n:
        raise ValueError(f"deg must have {n} entries, got {deg.numel()}")
    L = lib()
    with torch.cuda.device(dev):
        coeff = torch.empty(n, dtype=torch.float64, device=dev) if want_coeff else None
        mean = torch.empty(1, dtype=torch.float64, device=dev) if want_mean else None
        ws = _workspace(L.pp_graph_clustering_ws_bytes(), dev)
        check(L.pp_graph_clustering(_p(triads), _p(deg), n, _p(coeff), _p(mean), _p(ws), ws.numel(), _stream()), "pp_graph_clustering")
    return coeff, mean


# ------------------------------------------------------------------ colour refinement (pp_graph_wl.hip)
# Work split of the row walks, None = the library's choice (include/pathpyg_amd.h): the lanes per row (a power of two up to 64) and the row
# length from which a row gets a whole workgroup.  They change the time, never a result.
WL_GROUP: int | None = None
WL_HEAVY_MIN: int | None = None


def wl_heavy_min() -> int:
    """The row length from which colour refinement gives a row a whole workgroup (``WL_HEAVY_MIN`` or the library's default)."""
    return int(WL_HEAVY_MIN or lib().pp_graph_wl_heavy_min())


class WlStats(NamedTuple):
    counts: list            # counts[r]: classes after round r; counts[0]: distinct initial colours
    passes: list            # passes[r]: verify passes of round r
    seconds: "list | None"  # [keys + sort, new kernels, grouping] when timed


def graph_wl_refine(row_ptr: torch.Tensor, col: torch.Tensor, num_nodes: int, initial: torch.Tensor | None = None,
                    order: torch.Tensor | None = None, max_rounds: int | None = None, hash_mask: int = 0xFFFFFFFFFFFFFFFF, timed: bool = False):
    """Colour refinement on a CSR: ``(colours int64 [n] on the device, WlStats)``; see ``pp_graph_wl_refine`` in the header."""
    row_ptr, col = row_ptr.to(torch.int64).contiguous(), col.to(torch.int64).contiguous()
    n, m = int(num_nodes), col.numel()
    if row_ptr.numel() != n + 1:
        raise ValueError(f"row_ptr must have num_nodes + 1 = {n + 1} entries, got {row_ptr.numel()}")
    vectors = []
    for t, name in ((initial, "initial"), (order, "order")):
        if t is not None:
            if t.dtype != torch.int64 or t.numel() != n:
                raise ValueError(f"{name} must be an int64 vector of num_nodes = {n} entries")
            t = t.reshape(-1).contiguous()
        vectors.append(t)
    initial, order = vectors
    if max_rounds is not None and max_rounds < 0:
        raise ValueError("max_rounds must be None or >= 0")
    dev = require_device(row_ptr, col, initial, order)
    mask = int(hash_mask) & 0xFFFFFFFFFFFFFFFF
    mask = mask - (1 << 64) if mask >> 63 else mask                     # (the same 64 bits as an int64)
    cap = n + 2 if max_rounds is None else min(n, max_rounds) + 2
    L = lib()
    with torch.cuda.device(dev):
        colours = torch.empty(n, dtype=torch.int64, device=dev)
        counts, passes = (ctypes.c_int64 * cap)(), (ctypes.c_int64 * cap)()
        rounds = ctypes.c_int64(0)
        seconds = (ctypes.c_double * 3)() if timed else None
        ws = _workspace(L.pp_graph_wl_ws_bytes(n, m), dev)
        check(L.pp_graph_wl_refine(_p(row_ptr), _p(col), n, m, _p(initial), _p(order), -1 if max_rounds is None else int(max_rounds), mask,
                                   int(WL_GROUP or 0), int(WL_HEAVY_MIN or 0), _p(colours), ctypes.addressof(counts), ctypes.addressof(passes),
                                   cap, ctypes.addressof(rounds), ctypes.addressof(seconds) if timed else None, _p(ws), ws.numel(), _stream()),
              "pp_graph_wl_refine")
    r = rounds.value + 1
    return colours, WlStats(list(counts[:r]), list(passes[:r]), list(seconds) if timed else None)


# ------------------------------------------------------------------ power-iteration centralities (pp_graph_power.hip)
POWER_EIGENVECTOR, POWER_KATZ = 0, 1


def power_heavy_min() -> int:
    """The predecessor-list length from which the power iteration gives a row a whole workgroup (the library's default)."""
    return int(lib().pp_graph_power_heavy_min())


class PowerStats(NamedTuple):
    iterations: int         # iterations done
    converged: bool         # the L1 criterion held at that iteration
    light_grid: int         # workgroups of the light gather launch
    heavy_grid: int         # workgroups of the heavy gather launch (0: no row reached heavy_min)


def graph_power_iterate(col_ptr: torch.Tensor, row: torch.Tensor, weight: torch.Tensor | None, num_nodes: int, mode: int, threshold: float,
                        max_iter: int, alpha: float = 0.0, beta: torch.Tensor | float = 0.0, start: torch.Tensor | None = None,
                        normalized: bool = True, group: int = 0, heavy_min: int = 0, batch: int = 0):
    """Power iteration on predecessor lists: ``(values float64 [n] on the device, PowerStats)``; see ``pp_graph_power_iterate`` in the
    header.  ``group``, ``heavy_min`` and ``batch``: 0 = the library's choice."""
    col_ptr, row = col_ptr.to(torch.int64).contiguous(), row.to(torch.int64).contiguous()
    n, k = int(num_nodes), row.numel()
    if col_ptr.numel() != n + 1:
        raise ValueError(f"col_ptr must have num_nodes + 1 = {n + 1} entries, got {col_ptr.numel()}")
    beta_vec = beta if isinstance(beta, torch.Tensor) else None
    vectors = []
    for t, name, size in ((weight, "weight", k), (beta_vec, "beta", n), (start, "start", n)):
        if t is not None:
            if t.dtype != torch.float64 or t.numel() != size:
                raise ValueError(f"{name} must be a float64 vector of {size} entries")
            t = t.reshape(-1).contiguous()
        vectors.append(t)
    weight, beta_vec, start = vectors
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    dev = require_device(col_ptr, row, weight, beta_vec, start)
    L = lib()
    with torch.cuda.device(dev):
        values = torch.empty(n, dtype=torch.float64, device=dev)
        iterations, converged, grids = ctypes.c_int64(0), ctypes.c_int64(0), (ctypes.c_int64 * 2)()
        ws = _workspace(L.pp_graph_power_ws_bytes(n), dev)
        check(L.pp_graph_power_iterate(_p(col_ptr), _p(row), _p(weight), n, k, int(mode), float(alpha), _p(beta_vec),
                                       0.0 if beta_vec is not None else float(beta), _p(start), int(bool(normalized)), float(threshold),
                                       int(max_iter), int(batch), int(group), int(heavy_min), _p(values), ctypes.addressof(iterations),
                                       ctypes.addressof(converged), ctypes.addressof(grids), _p(ws), ws.numel(), _stream()),
              "pp_graph_power_iterate")
    return values, PowerStats(int(iterations.value), bool(converged.value), int(grids[0]), int(grids[1]))


# ------------------------------------------------------------------ node layouts (pp_graph_layout.hip)
LAYOUT_CIRCULAR, LAYOUT_GRID = 0, 1


def layout_heavy_min() -> int:
    """The neighbour-list length from which the layout iteration gives a node a whole workgroup (the library's default)."""
    return int(lib().pp_graph_layout_heavy_min())


class LayoutStats(NamedTuple):
    target_blocks: int      # grid x of the repulsion launch
    chunks: int             # grid y of the repulsion launch: the pieces of the source range
    light_grid: int         # workgroups of the light attraction launch
    heavy_grid: int         # workgroups of the heavy attraction launch (0: no node reached heavy_min)


def graph_layout_adjacency(edge_index: torch.Tensor, weight: torch.Tensor | None, num_nodes: int):
    """``(ptr int64 [n + 1], nbr int64 [nnz], w float64 [nnz])`` on the device: the symmetric adjacency of ``pp_graph_layout_adj_count`` /
    ``_fill`` in the header (last stored edge of a pair wins, self-loops dropped)."""
    ei = _edge_index(edge_index)
    n, m = int(num_nodes), ei.size(1)
    if weight is not None:
        if weight.numel() != m:
            raise ValueError(f"weight must have one value per stored edge ({m}), got {weight.numel()}")
        weight = weight.reshape(-1).to(torch.float64).contiguous()
    dev = require_device(ei, weight)
    L = lib()
    with torch.cuda.device(dev):
        nnz = ctypes.c_int64(0)
        ws = _workspace(L.pp_graph_layout_adj_ws_bytes(m), dev)
        check(L.pp_graph_layout_adj_count(_p(ei), m, n, ctypes.addressof(nnz), _p(ws), ws.numel(), _stream()), "pp_graph_layout_adj_count")
        k = int(nnz.value)
        ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        nbr = torch.empty(k, dtype=torch.int64, device=dev)
        w = torch.empty(k, dtype=torch.float64, device=dev)
        check(L.pp_graph_layout_adj_fill(_p(weight), m, n, k, _p(ptr), _p(nbr), _p(w), _p(ws), ws.numel(), _stream()), "pp_graph_layout_adj_fill")
    return ptr, nbr, w


def graph_layout_iterate(ptr: torch.Tensor, nbr: torch.Tensor, w: torch.Tensor | None, pos: torch.Tensor, k: float, t: float | None,
                         dt: float | None, iterations: int, threshold: float, fixed: torch.Tensor | None = None, block: int = 0,
                         chunks: int = 0, group: int = 0, heavy_min: int = 0, batch: int = 0):
    """Fruchterman-Reingold iterations from ``pos`` (float64 ``[n, 2]``, not modified): ``(new pos, iterations run, last err, LayoutStats)``;
    see ``pp_graph_layout_iterate`` in the header.  ``t is None``: the temperature and its step come from the extent of ``pos``, on the
    device.  ``block``, ``chunks``, ``group``, ``heavy_min`` and ``batch``: 0 = the library's choice."""
    n, nnz = pos.size(0), nbr.numel()
    if pos.dim() != 2 or pos.size(1) != 2 or pos.dtype != torch.float64:
        raise ValueError(f"pos must be float64 [n, 2], got {pos.dtype} {tuple(pos.shape)}")
    if ptr.numel() != n + 1:
        raise ValueError(f"ptr must have n + 1 = {n + 1} entries, got {ptr.numel()}")
    ptr, nbr = ptr.to(torch.int64).contiguous(), nbr.to(torch.int64).contiguous()
    if w is not None:
        if w.dtype != torch.float64 or w.numel() != nnz:
            raise ValueError(f"w must be a float64 vector of {nnz} entries")
        w = w.contiguous()
    if fixed is not None:
        if fixed.numel() != n:
            raise ValueError(f"fixed must have {n} entries")
        fixed = fixed.reshape(-1).to(torch.uint8).contiguous()
    dev = require_device(ptr, nbr, w, pos, fixed)
    L = lib()
    with torch.cuda.device(dev):
        out = pos.contiguous().clone()
        ran, err, grids = ctypes.c_int64(0), ctypes.c_double(0.0), (ctypes.c_int64 * 4)()
        ws = _workspace(L.pp_graph_layout_ws_bytes(n, int(block), int(chunks)), dev)
        check(L.pp_graph_layout_iterate(_p(ptr), _p(nbr), _p(w), n, nnz, _p(out), _p(fixed), float(k), 0.0 if t is None else float(t),
                                        0.0 if dt is None else float(dt), int(t is None), int(iterations), float(threshold), int(batch),
                                        int(block), int(chunks), int(group), int(heavy_min), ctypes.addressof(ran), ctypes.addressof(err),
                                        ctypes.addressof(grids), _p(ws), ws.numel(), _stream()), "pp_graph_layout_iterate")
    return out, int(ran.value), float(err.value), LayoutStats(*(int(g) for g in grids))


def graph_layout_rescale(pos: torch.Tensor, scale: float, center) -> torch.Tensor:
    """``networkx.rescale_layout(pos, scale) + center`` of float64 ``[n, 2]`` positions, in place."""
    dev = require_device(pos)
    L = lib()
    with torch.cuda.device(dev):
        ws = _workspace(L.pp_graph_layout_rescale_ws_bytes(), dev)
        check(L.pp_graph_layout_rescale(_p(pos), pos.size(0), float(scale), float(center[0]), float(center[1]), _p(ws), ws.numel(), _stream()),
              "pp_graph_layout_rescale")
    return pos


def graph_layout_start(seed: int, n: int, dom_size: float, center, given: torch.Tensor | None, has: torch.Tensor | None, device) -> torch.Tensor:
    """Start positions float64 ``[n, 2]``: ``given`` where ``has`` (or everywhere if ``has is None``), else ``uniform[0, 1) * dom_size + center``."""
    dev = torch.device(device)
    L = lib()
    with torch.cuda.device(dev):
        pos = torch.empty((n, 2), dtype=torch.float64, device=dev)
        check(L.pp_graph_layout_start(_i64(seed), n, float(dom_size), float(center[0]),
                                      float(center[1]), _p(given), _p(has), _p(pos), _stream()), "pp_graph_layout_start")
    return pos


def graph_layout_random(seed: int, n: int, center, device) -> torch.Tensor:
    """float32 ``[n, 2]`` uniform in ``[0, 1) + center``."""
    dev = torch.device(device)
    L = lib()
    with torch.cuda.device(dev):
        pos = torch.empty((n, 2), dtype=torch.float32, device=dev)
        check(L.pp_graph_layout_random(_i64(seed), n, float(center[0]), float(center[1]),
                                       _p(pos), _stream()), "pp_graph_layout_random")
    return pos


def graph_layout_closed_form(kind: int, n: int, device) -> torch.Tensor:
    """float64 ``[n, 2]``: the unit circle of ``networkx.circular_layout`` before its rescale, or the reference's grid."""
    dev = torch.device(device)
    L = lib()
    with torch.cuda.device(dev):
        pos = torch.empty((n, 2), dtype=torch.float64, device=dev)
        check(L.pp_graph_layout_closed_form(int(kind), n, _p(pos), _stream()), "pp_graph_layout_closed_form")
    return pos


# ------------------------------------------------------------------ DBGNN message passing
class CsrPlan:
    """CSR pair of one propagation: ``fwd`` rows are the destinations, ``bwd`` rows the sources (transposed)."""

    __slots__ = ("n_dst", "n_src", "fwd_ptr", "fwd_idx", "fwd_val", "bwd_ptr", "bwd_idx", "bwd_val", "self_coef", "fwd_heavy", "bwd_heavy",
                 "dst_order", "edge_ordered", "aug")          # edge_ordered: bwd_idx[e] is the destination of edge e (plan of a row-sorted edge list)

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


HEAVY_ROW_ENTRIES = 512      # CSR rows longer than this (hubs of scale-free graphs) are summed by the chunked pre-pass


class HeavyRows:
    """Hub rows of one CSR direction: ``slot`` [n_rows] int32 (-1 = ordinary row) and the chunk table of ``pp_spmm_heavy_f32``."""

    __slots__ = ("slot", "chunk_begin", "chunk_end", "chunk_ptr", "n_heavy", "n_chunks")

    def __init__(self, ptr: torch.Tensor, n_rows: int, threshold: int = HEAVY_ROW_ENTRIES):
        dev = ptr.device
        length = ptr[1:] - ptr[:-1]
        rows = torch.nonzero(length > threshold).flatten()
        self.n_heavy = int(rows.numel())
        chunk = int(lib().pp_heavy_chunk_entries())
        per_row = (length[rows].to(torch.int64) + chunk - 1) // chunk
        chunk_ptr = torch.zeros(self.n_heavy + 1, dtype=torch.int64, device=dev)
        chunk_ptr[1:] = torch.cumsum(per_row, 0)
        self.n_chunks = int(chunk_ptr[-1])
        owner = torch.repeat_interleave(torch.arange(self.n_heavy, device=dev), per_row)
        within = torch.arange(self.n_chunks, device=dev) - chunk_ptr[owner]
        begin = ptr[rows].to(torch.int64)[owner] + within * chunk
        end = torch.minimum(begin + chunk, ptr[rows + 1].to(torch.int64)[owner])
        self.chunk_begin, self.chunk_end = begin.to(torch.int32), end.to(torch.int32)
        self.chunk_ptr = chunk_ptr.to(torch.int32)
        self.slot = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
        self.slot[rows] = torch.arange(self.n_heavy, dtype=torch.int32, device=dev)

    def aggregate(self, idx: torch.Tensor, val: torch.Tensor | None, x: torch.Tensor) -> torch.Tensor:
        """``[n_heavy, F]`` neighbour sums of the hub rows over ``x`` (chunked, fixed summation order)."""
        f = x.size(1)
        L = lib()
        with torch.cuda.device(x.device):
            out = torch.empty((self.n_heavy, f), dtype=torch.float32, device=x.device)
            ws = _workspace(L.pp_spmm_heavy_ws_bytes(self.n_chunks, f), x.device)
            check(L.pp_spmm_heavy_f32(_p(idx), _p(val), _p(x), f, self.n_chunks, _p(self.chunk_begin), _p(self.chunk_end), self.n_heavy,
                                      _p(self.chunk_ptr), _p(out), _p(ws), ws.numel(), _stream()), "pp_spmm_heavy_f32")
        return out


def _heavy_args(heavy: "HeavyRows | None", idx, val, x):
    """(slot, sums) to hand to a row kernel; ``(None, None)`` for plans without hub rows or feature widths the pre-pass cannot take."""
    if heavy is None or x.size(1) % 4 != 0 or x.size(1) > 256:
        return None, None
    return heavy.slot, heavy.aggregate(idx, val, x.contiguous())


def _plan_report(ws: torch.Tensor) -> torch.Tensor:
    """Device int64 [3] = {status bits, longest forward row, longest backward row} of the plan a builder just queued on workspace ``ws``
    (pp_plan_result_ptr(ws)[1..3]: the kernels of the plan report the row lengths themselves, no extra launches)."""
    return ws[8:32].view(torch.int64).clone()


def _finish_plans(entries: list, what: str) -> list:
    """ONE device-to-host copy for everything the host must know about freshly built plans: the bad-index status and the longest
    rows (hub rows get their chunk tables here — the rare path, a few torch ops).  Returns ``[(status, longest forward row, longest
    backward row)]`` per plan."""
    if not entries:
        return []
    host = (entries[0][0] if len(entries) == 1 else torch.cat([report for report, _ in entries])).tolist()
    if any(int(host[3 * k]) & 1 for k in range(len(entries))):
        raise IndexError(f"{what}: node index out of range")
    for k, (_, plan) in enumerate(entries):
        if host[3 * k + 1] > HEAVY_ROW_ENTRIES:
            plan.fwd_heavy = HeavyRows(plan.fwd_ptr, plan.n_dst)
        if host[3 * k + 2] > HEAVY_ROW_ENTRIES:
            plan.bwd_heavy = HeavyRows(plan.bwd_ptr, plan.n_src)
    return [tuple(int(v) for v in host[3 * k: 3 * k + 3]) for k in range(len(entries))]


def gcn_plan(edge_index: torch.Tensor, edge_weight: torch.Tensor | None, num_nodes: int, row_sorted: bool | None = None,
             status_out: list | None = None, want_dst_order: bool = False) -> CsrPlan:
    """GCN normalisation of a weighted graph, once per graph (see pp_gcn_plan in the C header).
    ``row_sorted=None`` checks on the device whether the sources are non-decreasing (one tiny kernel + 8-byte read).
    ``status_out``: append the device status word instead of reading it now (the caller checks several plans with ONE
    device-to-host copy, see :func:`check_plan_status`)."""
    ei = _edge_index(edge_index)
    if row_sorted is None:
        row_sorted = ei.size(1) < 2 or is_sorted(ei[0])
    dev = require_device(ei, edge_weight)
    e = ei.size(1)
    if edge_weight is not None:
        edge_weight = edge_weight.to(torch.float32).contiguous()
        if edge_weight.numel() != e:
            raise ValueError("edge_weights must hold one value per edge")
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        plan = CsrPlan(n_dst=num_nodes, n_src=num_nodes,
                       fwd_ptr=torch.empty(num_nodes + 1, **i32), fwd_idx=torch.empty(e, **i32), fwd_val=torch.empty(e, **f32),
                       bwd_ptr=torch.empty(num_nodes + 1, **i32), bwd_idx=torch.empty(e, **i32), bwd_val=torch.empty(e, **f32),
                       self_coef=torch.empty(num_nodes, **f32))
        ws = _workspace(L.pp_gcn_plan_ws_bytes(e, num_nodes), dev)
        if want_dst_order:
            plan.dst_order = torch.empty(e, **i32)
        check(L.pp_gcn_plan(_p(ei), _p(edge_weight), e, num_nodes, 1 if row_sorted else 0, _p(plan.fwd_ptr), _p(plan.fwd_idx), _p(plan.fwd_val), _p(plan.bwd_ptr),
                            _p(plan.bwd_idx), _p(plan.bwd_val), _p(plan.self_coef), _p(plan.dst_order), _p(ws), ws.numel(), _stream()), "pp_gcn_plan")
        plan.edge_ordered = bool(row_sorted)
        entry = (_plan_report(ws), plan)
        if status_out is None:
            _finish_plans([entry], "GCNConv")
        else:
            status_out.append(entry)
    return plan


def gcn_plan_partition(edge_index_local: torch.Tensor, edge_weight: torch.Tensor | None, n_src: int, n_dst: int, halo_dinv,
                       row_sorted: bool = False, status_out: list | None = None, want_dst_order: bool = False) -> CsrPlan:
    """GCN plan of a DESTINATION-ROW PARTITION (multi-GPU DBGNN): ``edge_index_local`` [2, E] holds local ids — row 0 (sources) below
    ``n_src`` = owned + halo rows, row 1 (destinations) below ``n_dst`` = owned rows, owned node i is source i and destination i.
    ``halo_dinv(dinv_own [n_dst]) -> dinv_halo [n_src - n_dst]`` is called between the two phases of the plan (pp_gcn_plan_begin /
    pp_gcn_plan_finish) and returns the d^-1/2 of the halo rows from their owners (one 4-byte-per-row halo exchange)."""
    ei = _edge_index(edge_index_local)
    dev = require_device(ei, edge_weight)
    e = ei.size(1)
    if edge_weight is not None:
        edge_weight = edge_weight.to(torch.float32).contiguous()
        if edge_weight.numel() != e:
            raise ValueError("edge_weights must hold one value per edge")
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        plan = CsrPlan(n_dst=n_dst, n_src=n_src,
                       fwd_ptr=torch.empty(n_dst + 1, **i32), fwd_idx=torch.empty(e, **i32), fwd_val=torch.empty(e, **f32),
                       bwd_ptr=torch.empty(n_src + 1, **i32), bwd_idx=torch.empty(e, **i32), bwd_val=torch.empty(e, **f32),
                       self_coef=torch.empty(n_dst, **f32))
        dinv = torch.empty(n_src, **f32)
        ws = _workspace(L.pp_gcn_plan_ws_bytes(e, n_src), dev)
        if want_dst_order:
            plan.dst_order = torch.empty(e, **i32)
        rs = 1 if row_sorted else 0
        check(L.pp_gcn_plan_begin(_p(ei), _p(edge_weight), e, n_src, n_dst, rs, _p(plan.fwd_ptr), _p(plan.fwd_idx), _p(plan.fwd_val),
                                  _p(plan.bwd_ptr), _p(plan.self_coef), _p(dinv), _p(plan.dst_order), _p(ws), ws.numel(), _stream()),
              "pp_gcn_plan_begin")
        if halo_dinv is not None:            # a collective: called even when this rank has no halo rows
            dinv[n_dst:] = halo_dinv(dinv[:n_dst])
        check(L.pp_gcn_plan_finish(_p(ei), _p(edge_weight), e, n_src, n_dst, rs, _p(dinv), _p(plan.fwd_idx), _p(plan.fwd_val), _p(plan.bwd_ptr),
                                   _p(plan.bwd_idx), _p(plan.bwd_val), _p(ws), ws.numel(), _stream()), "pp_gcn_plan_finish")
        entry = (_plan_report(ws), plan)
        if status_out is None:
            _finish_plans([entry], "GCNConv (partition)")
        else:
            status_out.append(entry)
    return plan


_IDENTITY_PTR: dict = {}


def _identity_ptr(n: int, dev) -> torch.Tensor:
    """``arange(n + 1)`` as int32 row pointers (one entry per row), kept for the last size asked for on a device: the order-2 node count of
    consecutive batches of one stream rarely changes, and the array is read-only."""
    hit = _IDENTITY_PTR.get(dev)
    if hit is None or hit.numel() != n + 1:
        hit = torch.arange(n + 1, dtype=torch.int32, device=dev)
        _IDENTITY_PTR[dev] = hit
    return hit


def bipartite_plan_from_edge_grouping(plan_fo: CsrPlan, edge_dst: torch.Tensor, n_ho: int) -> CsrPlan:
    """Bipartite "last" plan of an order-2 De Bruijn model WITHOUT another sort: the higher-order nodes are the first-order graph's
    edges (same order), so "the higher-order nodes that end in node v" = "the edges into v" = the destination grouping the
    first-order GCN plan already holds (``gcn_plan(..., want_dst_order=True)``).  ``edge_dst`` = ``edge_index[1]`` of that graph."""
    dev = plan_fo.fwd_ptr.device
    ptr = plan_fo.fwd_ptr
    # (the plan of a row-sorted edge list already holds the destinations in edge order as its source-major index: no int32 copy)
    bwd_idx = plan_fo.bwd_idx if plan_fo.edge_ordered else edge_dst.to(torch.int32).contiguous()
    plan = CsrPlan(n_dst=plan_fo.n_dst, n_src=n_ho, fwd_ptr=ptr, fwd_idx=plan_fo.dst_order, fwd_val=None,
                   bwd_ptr=_identity_ptr(n_ho, dev), bwd_idx=bwd_idx, bwd_val=None,
                   self_coef=(ptr[1:] - ptr[:-1]).to(torch.float32))
    plan.fwd_heavy = plan_fo.fwd_heavy              # same row pointers: the same hub rows
    return plan


def check_plan_status(entries: list, what: str = "DBGNN") -> list:
    """One device-to-host copy for the status words (and longest rows) collected by several plan builders; returns
    ``[(status, longest forward row, longest backward row)]``."""
    return _finish_plans(entries, what)


def bipartite_plan(bipartite_index: torch.Tensor, n_ho: int, n_fo: int, pair_value: torch.Tensor | None = None,
                   src_sorted: bool | None = None, status_out: list | None = None) -> CsrPlan:
    """CSR pair of a [2, n_pairs] (source, destination) index between two node sets (``n_ho`` sources, ``n_fo``
    destinations); ``self_coef`` = in-degree of every destination.  ``pair_value``: optional coefficient per pair."""
    bi = _edge_index(bipartite_index)
    dev = require_device(bi, pair_value)
    nb = bi.size(1)
    if pair_value is not None:
        pair_value = pair_value.to(torch.float32).contiguous()
    if src_sorted is None:
        src_sorted = nb < 2 or is_sorted(bi[0])
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        plan = CsrPlan(n_dst=n_fo, n_src=n_ho,
                       fwd_ptr=torch.empty(n_fo + 1, **i32), fwd_idx=torch.empty(nb, **i32),
                       bwd_ptr=torch.empty(n_ho + 1, **i32), bwd_idx=torch.empty(nb, **i32),
                       self_coef=torch.empty(n_fo, **f32))
        if pair_value is not None:
            plan.fwd_val, plan.bwd_val = torch.empty(nb, **f32), torch.empty(nb, **f32)
        ws = _workspace(L.pp_gcn_plan_ws_bytes(nb, max(n_ho, n_fo)), dev)
        check(L.pp_bipartite_plan(_p(bi), nb, n_ho, n_fo, 1 if src_sorted else 0, _p(pair_value), _p(plan.fwd_ptr), _p(plan.fwd_idx), _p(plan.fwd_val),
                                  _p(plan.self_coef), _p(plan.bwd_ptr), _p(plan.bwd_idx), _p(plan.bwd_val), _p(ws), ws.numel(), _stream()),
              "pp_bipartite_plan")
        entry = (_plan_report(ws), plan)
        if status_out is None:
            _finish_plans([entry], "BipartiteGraphOperator")
        else:
            status_out.append(entry)
    return plan


_INT32_ROWS = 0x7ffffff0           # sizes the int32 CSR arrays of the order-2 builder can hold


class DeBruijn2:
    """Result of :func:`debruijn2`: the GCN plans of the first-order and the order-2 graph of a temporal stream, the bipartite "last" plan
    and the layer sizes (``m`` events, ``E2`` lifted instance pairs, ``U2`` order-2 nodes = first-order edges, ``A2`` order-2 edges)."""

    __slots__ = ("fo", "ho", "bip", "sizes", "fo_weight", "fo_dst", "ho_fwd_weight")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


_HUB_STATS = 8 + 2 * (64 + 1)          # index of the hub block inside the builder's int64 result header (csrc/pp_debruijn.hip: kDb2HubStats)
_HUB_PART_BYTES_MAX = 24 << 30         # per-task partial results of the hub nodes (768 bytes per part column): beyond this the generic kernels
_tls = threading.local()


_A2_GUESS: dict = {}                    # (m, n, want_weights, delta) -> A2 of the last build of a stream of that shape at that delta (debruijn2 allocates ahead of its read-back;
#                                         delta is part of the key: a sweep from a large to a small delta would otherwise keep plans that are views of buffers many times too long)


def _a2_buffers(a2: int, want_weights: bool, i32: dict, f32: dict) -> tuple:
    """The A2-sized outputs of :func:`debruijn2`: forward / backward index + value arrays, the 2 * A2 pack scratch, the raw weights."""
    return (torch.empty(a2, **i32), torch.empty(a2, **f32), torch.empty(a2, **i32), torch.empty(a2, **f32), torch.empty(2 * a2, **i32),
            torch.empty(a2, **f32) if want_weights else None)


def _pinned_stats() -> torch.Tensor:
    """Pinned int64 [16 + 154] of the calling thread: where pp_debruijn2_lists copies the hub statistics ([:16]) and pp_debruijn2_count the
    result header ([16:]), both asynchronously."""
    buf = getattr(_tls, "stats", None)
    if buf is None:
        buf = _tls.stats = torch.empty(16 + _HUB_STATS + 16, dtype=torch.int64).pin_memory()
    return buf


DENSE_EVENTS_PER_NODE = 2048


def debruijn2_wanted(m: int, num_nodes: int) -> bool:
    """Whether the node-by-node order-2 builder is the one to use for a stream of ``m`` events over ``num_nodes`` nodes.  It works node by node —
    in-events x out-events of the middle node — and is built for nodes with tens of events per side (hubs are chunked).  On a contact-shaped
    stream (tens of nodes, 10^4 events per node and side: 96 nodes / 2 * 10^6 events) every node is a hub and the per-node scans cost 1.9 ms where
    lift -> coalesce -> coalesce -> plans takes 1.0 ms (``hub_streams`` in the bench line): from ``DENSE_EVENTS_PER_NODE`` events per node on average
    the callers that choose (``MultiOrderModel.from_temporal_graph``, ``distributed.build_dbgnn_shard`` at world size 1) take the generic kernels.
    At world size > 1 ``build_dbgnn_shard`` does not ask: it always tries the node-range builder first."""
    return m <= DENSE_EVENTS_PER_NODE * max(int(num_nodes), 1)


def debruijn2(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int, delta, weight: torch.Tensor | None = None,
              want_weights: bool = False, unsorted_ok: bool = False):
    """Order-2 De Bruijn model of a TIME-SORTED event stream, fused (pp_debruijn2_lists / _count / _fill, csrc/pp_debruijn.hip): what
    ``coalesce`` (layer 1) + ``temporal_lift`` + ``coalesce`` (layer 2) + ``gcn_plan`` x 2 + ``bipartite_plan_from_edge_grouping`` build,
    identical array by array, without the event graph.  Two read-backs: the hub statistics (behind the sorts; the wait runs under the
    out-side kernel) and the layer sizes.  Nodes with more than 64 in- / out-events (hubs) are worked on chunk-wise by the same builder;
    rows of more than 512 entries get the chunk tables of the DBGNN kernels (``HeavyRows``).  ``weight``: None (unit weights) or float32 [m].
    ``want_weights``: also keep the merged order-2 weights themselves (``ho_fwd_weight`` [A2], destination-major order, beside the normalised
    coefficients of the plan) — what ``MultiOrderModel.layers[2].data.edge_weight`` is derived from when it is read.
    Returns a :class:`DeBruijn2`, or ``None`` when the builder does not apply (an empty stream, a weight vector that is not float32, more than
    2^31 order-2 edges, hub partials beyond 24 GiB; with ``unsorted_ok`` an unsorted stream): the caller then takes the generic path.
    Merged weights: layer 1 is the reference's left-to-right sum (the float64 sum rounded once from 2^24 on, exact counts for unit weights).
    Layer 2 through a hub node is summed in (in-event, task) order: equal to the reference's sum for integer-valued weights below 2^24,
    otherwise within (len - 1) * 2^-24 * sum|w| of the exact sum of an edge's len instances - the one association that differs."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, time, weight)
    stream = _event_stream(ei, time, weight)
    m, n = ei.size(1), int(num_nodes)
    if stream is None or m == 0 or n == 0:
        return None
    time, weight = stream
    kind, di, df = resolve_delta(time.dtype, delta)
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        ws = _workspace(L.pp_debruijn2_ws_bytes(m, n), dev)
        tcode = _DTYPE_CODE[time.dtype]
        stats = _pinned_stats()
        check(L.pp_debruijn2_lists(_p(ei), _p(time), tcode, m, n, _p(weight), _p(ws), ws.numel(), stats.data_ptr(), _stream()), "pp_debruijn2_lists")
        fo_bwd_ptr, fo_fwd_ptr = torch.empty(n + 1, **i32), torch.empty(n + 1, **i32)       # (allocated while the GPU sorts)
        fo_bwd_idx, fo_w = torch.empty(m, **i32), torch.empty(m, **f32)
        ho_fwd_ptr, ho_bwd_ptr = torch.empty(m + 1, **i32), torch.empty(m + 1, **i32)
        ho_deg, fo_deg = torch.empty(m, **f32), torch.empty(n, **f32)
        check(L.pp_debruijn2_wait(), "pp_debruijn2_wait")                                     # read-back 1 of 2: is there a hub node, how large
        hubs, packed, tasks, parts = (int(v) for v in stats[:4].tolist())
        out_hubs, out_events = packed >> 32, packed & 0xFFFFFFFF
        hub_ws = None
        if hubs:
            if parts * 768 > _HUB_PART_BYTES_MAX:
                return None
            hub_ws = _workspace(L.pp_debruijn2_hub_ws_bytes(out_events, out_hubs, parts), dev)
        hub_args = (hubs, out_hubs, out_events, tasks, parts, _p(hub_ws), hub_ws.numel() if hub_ws is not None else 0)
        check(L.pp_debruijn2_count(tcode, m, n, kind, di, df, _p(weight), _p(fo_bwd_ptr), _p(fo_bwd_idx), _p(fo_w), _p(fo_fwd_ptr), _p(ho_fwd_ptr),
                                   _p(ho_bwd_ptr), _p(ho_deg), _p(fo_deg), _p(ws), ws.numel(), *hub_args, stats.data_ptr() + 128, _stream()),
              "pp_debruijn2_count")
        # The outputs are allocated WHILE the count pass runs, not behind the read-back of its sizes (the GPU idles through everything the host
        # does between that read-back and the fill call): U2 = A1 <= m is a bound, A2 is guessed from the last build of a stream of this shape
        # (an epoch loop, a rolling window) and re-allocated when the guess is short or more than a quarter too long.
        ho_self, fo_fwd_idx, fo_fwd_val = torch.empty(m, **f32), torch.empty(m, **i32), torch.empty(m, **f32)
        fo_dst_order, fo_bwd_val, fo_self = torch.empty(m, **i32), torch.empty(m, **f32), torch.empty(n, **f32)
        guess_key = (m, n, want_weights, kind, di, df)
        guess = _A2_GUESS.get(guess_key, 0)
        a2_bufs = _a2_buffers(guess, want_weights, i32, f32) if guess else None
        launched = False
        if a2_bufs is not None:
            # .. and with a guess the fill is launched by the SAME C call that waits for the sizes (when the stream is good and A2 fits): no host
            # code between read-back and fill
            flag = stats[15:16]
            check(L.pp_debruijn2_fill_ready(tcode, m, n, kind, di, df, _p(weight), _p(fo_bwd_ptr), _p(fo_bwd_idx), _p(fo_w), _p(fo_fwd_ptr), _p(ho_fwd_ptr),
                                            _p(ho_bwd_ptr), _p(ho_deg), _p(fo_deg), guess, _p(a2_bufs[0]), _p(a2_bufs[1]), _p(a2_bufs[2]), _p(a2_bufs[3]),
                                            _p(ho_self), _p(fo_fwd_idx), _p(fo_fwd_val), _p(fo_dst_order), _p(fo_bwd_val), _p(fo_self), _p(a2_bufs[5]),
                                            _p(a2_bufs[4]), _p(ws), ws.numel(), *hub_args, 1, stats.data_ptr() + 128, flag.data_ptr(), _stream()),
                  "pp_debruijn2_fill_ready")
            launched = bool(int(flag[0]))
        else:
            check(L.pp_debruijn2_wait(), "pp_debruijn2_wait")                                 # read-back 2 of 2: the layer sizes (+ the hubs' share)
        head = stats[16:].tolist()
        u2, status, a2, e2, a1 = head[:5]
        e2 += head[_HUB_STATS + 4]
        longest = head[_HUB_STATS + 5: _HUB_STATS + 9] if hubs else (0, 0, 0, 0)
        _bad_index(status, "MultiOrderModel.from_temporal_graph")
        if status & 2:
            if unsorted_ok:           # (the caller sorts and takes the generic path: MultiOrderModel.from_temporal_graph, multi_order_model.py:148-151)
                return None
            raise ValueError("lift_order_temporal: the events are not sorted by time (TemporalGraph sorts them on construction; "
                             "data.time / data.edge_index were modified afterwards)")
        if status & 4:
            return None
        if a2 >= _INT32_ROWS:           # the builder's row pointers are int32 (the scan's TOTAL is int64, so this is the true A2): generic kernels
            return None
        if not launched and (a2_bufs is None or not (a2 <= guess <= a2 + a2 // 4 + 1024)):
            a2_bufs = _a2_buffers(a2, want_weights, i32, f32)
        if len(_A2_GUESS) >= 64 and guess_key not in _A2_GUESS:      # (a handful of stream shapes at a time: drop the oldest)
            _A2_GUESS.pop(next(iter(_A2_GUESS)))
        _A2_GUESS[guess_key] = a2
        ho_fwd_idx, ho_fwd_val, ho_bwd_idx, ho_bwd_val, pack, ho_fwd_w = (None if b is None else b[:k * a2] for b, k in zip(a2_bufs, (1, 1, 1, 1, 2, 1)))
        ho = CsrPlan(n_dst=u2, n_src=u2, fwd_ptr=ho_fwd_ptr[: u2 + 1], fwd_idx=ho_fwd_idx, fwd_val=ho_fwd_val,
                     bwd_ptr=ho_bwd_ptr[: u2 + 1], bwd_idx=ho_bwd_idx, bwd_val=ho_bwd_val, self_coef=ho_self[:u2], edge_ordered=True)
        fo = CsrPlan(n_dst=n, n_src=n, fwd_ptr=fo_fwd_ptr, fwd_idx=fo_fwd_idx[:a1], fwd_val=fo_fwd_val[:a1],
                     bwd_ptr=fo_bwd_ptr, bwd_idx=fo_bwd_idx[:u2], bwd_val=fo_bwd_val[:u2], self_coef=fo_self,
                     dst_order=fo_dst_order[:a1], edge_ordered=True)
        if not launched:
            check(L.pp_debruijn2_fill(tcode, m, n, kind, di, df, _p(weight), _p(fo_bwd_ptr), _p(fo_bwd_idx), _p(fo_w), _p(fo_fwd_ptr), _p(ho_fwd_ptr),
                                      _p(ho_bwd_ptr), _p(ho_deg), _p(fo_deg), a2, _p(ho.fwd_idx), _p(ho.fwd_val), _p(ho.bwd_idx), _p(ho.bwd_val),
                                      _p(ho.self_coef), _p(fo.fwd_idx), _p(fo.fwd_val), _p(fo.dst_order), _p(fo.bwd_val), _p(fo.self_coef), _p(ho_fwd_w),
                                      _p(pack), _p(ws), ws.numel(), *hub_args, 1, _stream()),
                  "pp_debruijn2_fill")
        # hub rows of the plans (more than 512 entries): the chunk tables of the row kernels' pre-pass, as pp_gcn_plan's report triggers them
        if longest[0] > HEAVY_ROW_ENTRIES:
            ho.fwd_heavy = HeavyRows(ho.fwd_ptr, u2)
        if longest[1] > HEAVY_ROW_ENTRIES:
            ho.bwd_heavy = HeavyRows(ho.bwd_ptr, u2)
        if longest[2] > HEAVY_ROW_ENTRIES:
            fo.fwd_heavy = HeavyRows(fo.fwd_ptr, n)
        if longest[3] > HEAVY_ROW_ENTRIES:
            fo.bwd_heavy = HeavyRows(fo.bwd_ptr, n)
    bip = bipartite_plan_from_edge_grouping(fo, None, u2)
    return DeBruijn2(fo=fo, ho=ho, bip=bip, fo_weight=fo_w[:u2], fo_dst=fo.bwd_idx, ho_fwd_weight=ho_fwd_w,
                     sizes={"m": m, "N": n, "E2": e2, "U2": u2, "A1": a1, "A2": a2, "hub_nodes": hubs, "hub_tasks": tasks})


class MultiOrderLayer:
    """One De Bruijn layer as source-major CSR (:func:`multi_order_temporal`): ``row_ptr`` int32 [n_nodes + 1], ``col`` int32 [n_edges], ``weight``
    float32 [n_edges] (merged weights), ``last`` int32 [n_edges] (last first-order node of every edge = of every node of the next layer; ``None``
    for the top layer of a build)."""

    __slots__ = ("n_nodes", "n_edges", "n_instances", "row_ptr", "col", "weight", "last")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def multi_order_temporal(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int, delta, weight: torch.Tensor | None, max_order: int,
                         clock: list | None = None, event_graph: torch.Tensor | None = None, pass_instances: int = _INT32_ROWS,
                         passes: list | None = None, unsorted_ok: bool = False):
    """All De Bruijn layers 1..max_order of a TIME-SORTED event stream, level by level (pp_multiorder_prepare / _step, csrc/pp_multiorder.hip):
    no instance graph ``[2, E_k]``, no per-instance node sequences, no global sort beyond the two of the first order; one read-back per order.
    Returns ``[MultiOrderLayer]`` (index k - 1 = layer k; ``n_instances`` = E_k, the instance edges the reference would have lifted, a Python
    int of any size) or ``None`` when the generic kernels have to take over: a layer without edges, a node sequence with more than 4096
    continuations (dense contact streams), a layer with 2^31 - 16 or more edges, 2^31 continuations of one first-order node pair and, with
    ``unsorted_ok``, a stream that is not sorted by time (torch.sort's order: a NaN before a number is a descent) — without it that stream
    raises ``ValueError``, as in :func:`temporal_lift` and :func:`debruijn2`.  A level with more than ``pass_instances`` instances (at most and by default what one step numbers, 2^31 - 17) is no refusal: from there
    on every level is cut into parts of whole types of at most that many instances, the unchanged step runs on one part after another and
    the parts' pieces are joined (``core/multi_order_passes.py``: pp_multiorder_split / _concat; one read-back per part and step, one per
    split).  ``passes``: a list that receives the number of parts layer 1..max_order were built in (all ones without such a level).
    ``clock``: a list that receives one ``(name, start event, end event)`` per phase — the windows and level 1 ("prepare"), then every
    step ("layer k", one per part; in passes also "split k" and "concat k") — for measurements (bench.py).  ``event_graph``: a given ``lift_order_temporal(g, delta)`` ([2, E2]
    int64, sorted by source) instead of ``time`` / ``delta`` (pp_multiorder_prepare_graph)."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, time, weight, event_graph)

    def tick():
        if clock is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev
    stream = _event_stream(ei, time, weight)
    m, n = ei.size(1), int(num_nodes)
    if stream is None or m == 0 or n == 0 or m >= _INT32_ROWS:
        return None
    time, weight = stream
    kind, di, df = resolve_delta(time.dtype, delta)
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        t0 = tick()
        if event_graph is None:
            lift_ws = _workspace(L.pp_temporal_ws_bytes(m, n), dev)
            check(L.pp_temporal_windows(_p(ei), _p(time), _DTYPE_CODE[time.dtype], m, n, kind, di, df, _p(lift_ws), lift_ws.numel(), _stream()),
                  "pp_temporal_windows")
            n_list = m
        else:
            eg = _edge_index(event_graph)
            n_list = eg.size(1)
            if n_list == 0 or n_list >= _INT32_ROWS:
                return None
            lift_ws = _workspace(L.pp_multiorder_graph_ws_bytes(m, n_list), dev)
        tab = torch.empty((n_list, 4), **i32)
        inst = torch.empty((m, 4), **i32)
        tptr, ibase = torch.empty(m + 1, **i32), torch.empty(m + 1, **i32)
        tlast, w = torch.empty(m, **i32), torch.empty(m, **f32)
        row_ptr = torch.empty(n + 1, **i32)
        ws = _workspace(L.pp_multiorder_prepare_ws_bytes(m), dev)
        # the (source, target, time) order of the events: every node's out-list sorted in LDS; a node with more than 4096 out-events (status bit 4:
        # its list is left unsorted) sends the stream to the radix sort — contact-shaped streams go there at once
        for radix in ((True,) if (event_graph is not None or m > 1024 * n) else (False, True)):
            if event_graph is None:
                check(L.pp_multiorder_prepare(_p(ei), m, n, _p(weight), _p(lift_ws), lift_ws.numel(), 1 if radix else 0, _p(tab), _p(inst), _p(tptr),
                                              _p(ibase), _p(tlast), _p(w), _p(row_ptr), _p(ws), ws.numel(), _stream()), "pp_multiorder_prepare")
            else:
                check(L.pp_multiorder_prepare_graph(_p(ei), m, n, _p(weight), _p(eg), n_list, _p(lift_ws), lift_ws.numel(), _p(tab), _p(inst), _p(tptr),
                                                    _p(ibase), _p(tlast), _p(w), _p(row_ptr), _p(ws), ws.numel(), _stream()), "pp_multiorder_prepare_graph")
            types, status, children, _ = ws[:32].view(torch.int64).tolist()
            if not status & 16:
                break
        if clock is not None:
            clock.append(("prepare", t0, tick()))
        del lift_ws, ws
        _bad_index(status, "MultiOrderModel.from_temporal_graph")
        if status & 2 and not unsorted_ok:
            raise ValueError("lift_order_temporal: the events are not sorted by time (TemporalGraph sorts them on construction; "
                             "data.time / data.edge_index were modified afterwards)")
        if status & (2 | 4):
            return None                  # (unsorted: the caller sorts and takes the generic path; 2^31 continuations of one node pair's events)
        if event_graph is not None and children != n_list:      # the instances of level 2 ARE the event graph's edges
            return None
        level = MultiOrderLevel(types=types, children=children, status=status, tptr=tptr, ibase=ibase, inst=inst, row_ptr=row_ptr, col=tlast,
                                weight=w, tlast=tlast)
        layers = [MultiOrderLayer(n_nodes=n, n_edges=types, n_instances=m, row_ptr=row_ptr, col=tlast[:types], weight=w[:types], last=tlast[:types])]
        cand_ptr, cand_last = row_ptr, tlast
        budget = max(1, min(int(pass_instances), _INT32_ROWS - 1))    # (a step numbers at most _INT32_ROWS - 1 children)
        if passes is not None:
            passes[:] = [1] * max_order
        for k in range(2, max_order + 1):
            if level.types == 0 or level.children == 0:
                return None
            if level.children > budget:
                # more instances than one step numbers (or than the caller's budget): the rest of the model in passes over ranges of types
                from .core import multi_order_passes
                built = multi_order_passes.continue_in_passes(sys.modules[__name__], level, cand_ptr, cand_last, tab, layers, max_order,
                                                              weight is not None, budget, clock)
                if built is None:
                    return None
                if passes is not None:
                    passes[k - 1:] = built[1]
                return built[0]
            last = k == max_order
            nxt = _multi_order_step(level, cand_ptr, cand_last, tab, weight is not None, last, clock, f"layer {k}")
            if nxt.status & 4:
                return None
            layers.append(MultiOrderLayer(n_nodes=level.types, n_edges=nxt.types, n_instances=level.children, row_ptr=nxt.row_ptr, col=nxt.col[:nxt.types],
                                          weight=nxt.weight[:nxt.types], last=None if last else nxt.tlast[:nxt.types]))
            cand_ptr, cand_last = nxt.row_ptr, nxt.tlast
            level = nxt
    return layers


def multi_order_paths(node_sequence: torch.Tensor, dag_num_nodes: torch.Tensor, dag_weight: torch.Tensor, edge_index: torch.Tensor, num_nodes: int,
                      max_order: int, want_inverse=True, clock: list | None = None):
    """All De Bruijn layers 1..max_order of OBSERVED WALKS (``PathData``'s tensors: ``node_sequence`` [P] or [P, 1] int64, ``dag_num_nodes`` [W]
    int64, ``dag_weight`` [W] float32, ``edge_index`` [2, P - W] int64; propagation mode), level by level: pp_multiorder_prepare_paths makes
    level 1 straight from the walk store, the unchanged pp_multiorder_step every further one, pp_multiorder_paths_inverse the ``inverse_idx`` of a
    layer from the level below it while that level's instances are alive.  ``num_nodes``: 1 + the largest node id.  Returns ``(layers,
    inverses)``: ``[MultiOrderLayer]`` as :func:`multi_order_temporal` and ``{k: int32 [instances of level k - 1]}`` for the layers k >= 2
    (``want_inverse``: True = all, "top" = layer ``max_order`` only, False = none) — or ``None`` when the generic kernels have to take over: node
    ids that are not exactly 0 .. num_nodes - 1, an ``edge_index`` that is not the chain of these walks (status bits 3 / 5), a layer without
    edges below ``max_order``, a node sequence observed at more than 4096 walk positions that all continue, 2^31 or more instances.
    ``clock`` receives ``(name, start event, end event)`` for "prepare", every "layer k" and every "inverse k"."""
    ei = _edge_index(edge_index)
    seq = node_sequence.reshape(-1).contiguous()
    lengths, weight = dag_num_nodes.contiguous(), dag_weight.contiguous()
    dev = require_device(ei, seq, lengths, weight)
    if seq.dtype != torch.int64 or lengths.dtype != torch.int64 or weight.dtype != torch.float32:
        raise TypeError("multi_order_paths: node_sequence / dag_num_nodes int64 and dag_weight float32 expected")
    positions, walks, m, n = seq.numel(), lengths.numel(), ei.size(1), int(num_nodes)
    if m == 0 or n <= 0 or walks == 0 or weight.numel() != walks or m != positions - walks or positions >= _INT32_ROWS or n >= 1 << 31:
        return None

    def tick():
        if clock is None:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        t0 = tick()
        tab, inst = torch.empty((m, 4), **i32), torch.empty((m, 4), **i32)
        tptr, ibase = torch.empty(m + 1, **i32), torch.empty(m + 1, **i32)
        tlast, w, edge_walk = torch.empty(m, **i32), torch.empty(m, **f32), torch.empty(m, **i32)
        row_ptr = torch.empty(n + 1, **i32)
        ws = _workspace(L.pp_multiorder_paths_ws_bytes(positions, walks, n), dev)
        check(L.pp_multiorder_prepare_paths(_p(seq), positions, _p(lengths), _p(weight), walks, _p(ei), m, n, _p(tab), _p(inst), _p(tptr), _p(ibase),
                                            _p(tlast), _p(w), _p(row_ptr), _p(edge_walk), _p(ws), ws.numel(), _stream()), "pp_multiorder_prepare_paths")
        types, status, children, _ = ws[:32].view(torch.int64).tolist()
        if clock is not None:
            clock.append(("prepare", t0, tick()))
        del ws
        if status & (8 | 32 | 4 | 16):
            return None                  # (ids with gaps or a foreign edge_index: the generic route; 2^31 continuations)
        level = MultiOrderLevel(types=types, children=children, status=status, tptr=tptr, ibase=ibase, inst=inst, row_ptr=row_ptr, col=tlast,
                                weight=w, tlast=tlast)
        layers = [MultiOrderLayer(n_nodes=n, n_edges=types, n_instances=m, row_ptr=row_ptr, col=tlast[:types], weight=w[:types], last=tlast[:types])]
        inverses = {}
        cand_ptr, cand_last = row_ptr, tlast
        instances = m
        inv_ws = _workspace(L.pp_multiorder_paths_inverse_ws_bytes(walks), dev) if want_inverse else None
        for k in range(2, max_order + 1):
            if level.types == 0 or level.children == 0 or level.children >= _INT32_ROWS:
                return None
            if want_inverse is True or (want_inverse == "top" and k == max_order):
                t0 = tick()
                inverse = torch.empty(instances, **i32)
                check(L.pp_multiorder_paths_inverse(k - 1, level.types, instances, _p(level.tptr), _p(level.inst), _p(edge_walk), m, _p(lengths), walks,
                                                    _p(inverse), _p(inv_ws), inv_ws.numel(), _stream()), "pp_multiorder_paths_inverse")
                inverses[k] = inverse
                if clock is not None:
                    clock.append((f"inverse {k}", t0, tick()))
            last = k == max_order
            nxt = _multi_order_step(level, cand_ptr, cand_last, tab, True, last, clock, f"layer {k}")
            if nxt.status & 4:
                return None
            layers.append(MultiOrderLayer(n_nodes=level.types, n_edges=nxt.types, n_instances=level.children, row_ptr=nxt.row_ptr, col=nxt.col[:nxt.types],
                                          weight=nxt.weight[:nxt.types], last=None if last else nxt.tlast[:nxt.types]))
            cand_ptr, cand_last = nxt.row_ptr, nxt.tlast
            instances = level.children
            level = nxt
    return layers, inverses


class MultiOrderLevel:
    """Level k of the level-by-level builder on the device, with layer k as it left the kernels: ``types`` types (= edges of layer k) with
    ``children`` instances at level k + 1 (both on the host, with ``status``, from the level's one read-back); ``tptr`` / ``ibase`` [types + 1],
    ``inst`` the level's instance records, ``tlast`` [types] the types' last nodes (``None`` for the top layer); layer k's ``row_ptr`` (over ITS
    nodes), ``col`` and ``weight`` (capacity >= types).  On a rank of the split by first node ``tptr`` / ``ibase`` / ``row_ptr`` are numbered from
    0 on the rank, ``col`` holds global ids."""

    __slots__ = ("types", "children", "status", "tptr", "ibase", "inst", "row_ptr", "col", "weight", "tlast")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def multi_order_step(level: MultiOrderLevel, cand_ptr: torch.Tensor, cand_last: torch.Tensor, tab: torch.Tensor, weighted: bool, last: bool,
                     clock: list | None = None, name: str = "layer") -> MultiOrderLevel:
    """Level k + 1 (and layer k + 1) from ``level`` = level k with ``types > 0`` types and ``children > 0`` children (pp_multiorder_step; one
    read-back).  ``cand_ptr`` / ``cand_last``: row pointers of layer k over ALL its nodes and the last nodes of ALL its edges — the tables a new
    edge's column ``suffix(s) ++ d`` is looked up in; the columns written are positions in them, so with the global tables a rank's own types
    (``tptr`` / ``ibase`` numbered from 0 on the rank) yield global columns.  ``last``: the top layer (no next level is kept).  Status bit 2:
    a type with more than 4096 children, the outputs are incomplete."""
    with torch.cuda.device(level.tptr.device):
        return _multi_order_step(level, cand_ptr, cand_last, tab, weighted, last, clock, name)


def _multi_order_step(level: MultiOrderLevel, cand_ptr, cand_last, tab, weighted: bool, last: bool, clock, name: str) -> MultiOrderLevel:
    """:func:`multi_order_step` under the caller's device guard (:func:`multi_order_temporal` holds one over all its levels)."""
    dev = level.tptr.device
    types, children = level.types, level.children
    L = lib()
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    child = torch.empty((children, (2 if weighted else 1) if last else 4), **i32)      # (the top layer's children are nobody's parents)
    row_next = torch.empty(types + 1, **i32)
    col_next, w_next = torch.empty(children, **i32), torch.empty(children, **f32)
    tptr_next = ibase_next = tlast_next = None
    if not last:
        tptr_next, ibase_next, tlast_next = torch.empty(children + 1, **i32), torch.empty(children + 1, **i32), torch.empty(children, **i32)
    ws = _workspace(L.pp_multiorder_step_ws_bytes(types, children), dev)
    t0 = None
    if clock is not None:
        t0 = torch.cuda.Event(enable_timing=True)
        t0.record()
    check(L.pp_multiorder_step(types, children, _p(level.tptr), _p(level.ibase), _p(level.col), _p(level.inst), _p(cand_ptr), _p(cand_last), _p(tab),
                               1 if weighted else 0, 1 if last else 0, _p(child), _p(row_next), _p(tptr_next), _p(ibase_next),
                               _p(tlast_next), _p(col_next), _p(w_next), _p(ws), ws.numel(), _stream()), "pp_multiorder_step")
    if clock is not None:
        t1 = torch.cuda.Event(enable_timing=True)
        t1.record()
        clock.append((name, t0, t1))
    new_types, status, new_children, _ = ws[:32].view(torch.int64).tolist()
    del ws
    if not status & 4 and 2 * new_types < children:                    # far fewer types than instances: do not keep the instance-sized buffers alive
        col_next, w_next = col_next[:new_types].clone(), w_next[:new_types].clone()
        if not last:
            tlast_next = tlast_next[:new_types].clone()
    return MultiOrderLevel(types=new_types, children=new_children, status=status, tptr=tptr_next, ibase=ibase_next, inst=child, row_ptr=row_next,
                           col=col_next, weight=w_next, tlast=tlast_next)


SPLIT_MAX_PARTS = 65536            # kMoSplitMaxParts of csrc/pp_multiorder.hip: parts one pp_multiorder_split makes


def multi_order_split(level: MultiOrderLevel, budget: int) -> "list[MultiOrderLevel] | None":
    """``level`` cut into parts of whole types with at most ``budget`` children each (pp_multiorder_split; one read-back): a part that starts
    at type t0 ends before the first type whose children would take it past the budget, holds at least one type, and a single type above
    the budget is a part of its own.  ``level.ibase`` may be wrapped (``level.children`` >= 2^31, the true count from the step's read-back):
    the per-type counts are its unsigned differences, their prefix is int64.  Every part is a :class:`MultiOrderLevel` that
    :func:`multi_order_step` takes as it is: ``tptr`` / ``ibase`` numbered from 0, ``inst`` / ``col`` / ``tlast`` / ``weight`` VIEWS of the
    level's arrays, ``children`` a Python int, ``row_ptr`` None.  ``None``: a single type with 2^31 or more children.  ``ValueError``: a
    budget so small that the level may need more than ``SPLIT_MAX_PARTS`` parts.  ``HipError``: ``ibase`` is not the (low 32 bits of the)
    prefix of ``level.children`` counts below 2^31."""
    dev = level.tptr.device
    types, children, budget = int(level.types), int(level.children), int(budget)
    if types <= 0 or budget < 1:
        raise ValueError("multi_order_split: a level with types and a budget >= 1")
    cap = min(types, 2 * (children // budget) + 2)         # (two neighbouring parts together exceed the budget)
    if cap > SPLIT_MAX_PARTS:
        raise ValueError(f"multi_order_split: {children} instances in parts of {budget} may need {cap} parts; one split makes at most {SPLIT_MAX_PARTS} "
                         "(its cuts are walked one after another: it is meant for two to a few hundred parts) — raise the budget")
    L = lib()
    with torch.cuda.device(dev):
        report = torch.empty(4 + 3 * (cap + 1), dtype=torch.int64, device=dev)
        tptr = torch.empty(types + cap, dtype=torch.int32, device=dev)
        ibase = torch.empty(types + cap, dtype=torch.int32, device=dev)
        ws = _workspace(L.pp_multiorder_split_ws_bytes(types), dev)
        check(L.pp_multiorder_split(types, _p(level.tptr), _p(level.ibase), budget, cap, _p(report), _p(tptr), _p(ibase), _p(ws), ws.numel(), _stream()),
              "pp_multiorder_split")
        host = report.tolist()
    parts, status, total = host[0], host[1], host[2]
    if status & 2:
        return None
    if status or total != children or not 1 <= parts <= cap:
        raise HipError(f"pp_multiorder_split: status {status}, {parts} parts (room for {cap}), {total} children counted, {children} expected")
    cut_type, cut_child, cut_inst = (host[4 + r * (cap + 1): 4 + r * (cap + 1) + parts + 1] for r in range(3))
    out = []
    for p in range(parts):
        t0, t1, i0, i1, at = cut_type[p], cut_type[p + 1], cut_inst[p], cut_inst[p + 1], cut_type[p] + p
        out.append(MultiOrderLevel(types=t1 - t0, children=cut_child[p + 1] - cut_child[p], status=0, tptr=tptr[at: at + t1 - t0 + 1],
                                   ibase=ibase[at: at + t1 - t0 + 1], inst=level.inst[i0:i1], row_ptr=None, col=level.col[t0:t1],
                                   weight=None if level.weight is None else level.weight[t0:t1],
                                   tlast=None if level.tlast is None else level.tlast[t0:t1]))
    return out


def multi_order_concat(pieces: list, want_last: bool):
    """The layer pieces of a level's parts, in part order, joined into the layer's global arrays (pp_multiorder_concat, no read-back):
    ``pieces`` = ``[(rows, level)]`` with ``level`` what :func:`multi_order_step` returned for the part of ``rows`` types (``row_ptr`` =
    offsets into its own edges, ``col`` / ``weight`` / ``tlast`` of ``level.types`` edges) or ``None`` for a part without children: ``rows``
    empty rows.  Returns ``(row_ptr int32 [sum rows + 1], col int32, weight float32, last int32 or None)``; ``want_last`` False: the top layer.
    ``ValueError`` / ``HipError``: a layer with 2^31 or more rows or edges."""
    filled = [b for _, b in pieces if b is not None]
    if not filled:
        raise ValueError("multi_order_concat: no piece with edges")
    dev = filled[0].row_ptr.device
    k = len(pieces)
    rows, edges = [int(r) for r, _ in pieces], [0 if b is None else int(b.types) for _, b in pieces]
    n_rows, n_edges = sum(rows), sum(edges)
    ptrs = ctypes.c_void_p * k

    def table(get):
        return ptrs(*[(get(b).data_ptr() if e else None) for e, (_, b) in zip(edges, pieces)])
    with torch.cuda.device(dev):
        row_ptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
        col = torch.empty(n_edges, dtype=torch.int32, device=dev)
        weight = torch.empty(n_edges, dtype=torch.float32, device=dev)
        last = torch.empty(n_edges, dtype=torch.int32, device=dev) if want_last else None
        for r, b in pieces:
            if b is None:
                continue
            if b.row_ptr.dtype != torch.int32 or b.row_ptr.numel() < r or (b.types and (b.col.dtype != torch.int32 or b.weight.dtype != torch.float32
                                                                 or b.col.numel() < b.types or b.weight.numel() < b.types
                                                                 or (want_last and b.tlast.numel() < b.types))):
                raise ValueError("multi_order_concat: a piece's arrays are not int32 / float32 of its sizes")
        check(lib().pp_multiorder_concat(k, ptrs(*[(None if b is None else b.row_ptr.data_ptr()) for _, b in pieces]), table(lambda b: b.col), table(lambda b: b.weight),
                                         table(lambda b: b.tlast) if want_last else None, (ctypes.c_int64 * k)(*rows), (ctypes.c_int64 * k)(*edges),
                                         _p(row_ptr), _p(col), _p(weight), _p(last), _stream()), "pp_multiorder_concat")
    return row_ptr, col, weight, last


def multi_order_node_loads(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int, delta, weight: torch.Tensor | None = None):
    """First step of the split by first node (:func:`pathpyg_amd.distributed.build_multi_order_shard`) on a replicated TIME-SORTED stream: the
    windows pass (pp_temporal_windows, whole stream) and the per-node loads the cuts are chosen from (pp_multiorder_node_loads).  Returns
    ``(windows, loads)``: ``windows`` is what :func:`multi_order_prepare_range` takes, ``loads`` int64 [2, num_nodes + 1] stays on the device —
    ``loads[0][v]`` = out-events of the nodes below v, ``loads[1][v]`` = level-2 instances that start at a node below v.  No read-back.
    ``None``: a stream the level-by-level builder does not take (empty, 2^31 events, not sorted by time, a weight that is not float32,
    tensors on the host)."""
    ei = _edge_index(edge_index)
    if not ei.is_cuda or not time.is_cuda or (weight is not None and not weight.is_cuda):
        return None
    dev = require_device(ei, time, weight)
    stream = _event_stream(ei, time, weight)
    m, n = ei.size(1), int(num_nodes)
    if stream is None or m == 0 or n == 0 or m >= _INT32_ROWS:
        return None
    time, weight = stream
    if not is_sorted(time):              # (one cheap kernel instead of the windows pass; replicated input: every rank decides alike)
        return None
    kind, di, df = resolve_delta(time.dtype, delta)
    L = lib()
    with torch.cuda.device(dev):
        lift_ws = _workspace(L.pp_temporal_ws_bytes(m, n), dev)
        check(L.pp_temporal_windows(_p(ei), _p(time), _DTYPE_CODE[time.dtype], m, n, kind, di, df, _p(lift_ws), lift_ws.numel(), _stream()),
              "pp_temporal_windows")
        loads = torch.empty((2, n + 1), dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_multiorder_node_loads_ws_bytes(m), dev)
        check(L.pp_multiorder_node_loads(m, n, _p(lift_ws), lift_ws.numel(), _p(loads), _p(ws), ws.numel(), _stream()), "pp_multiorder_node_loads")
    return (ei, weight, n, lift_ws), loads


def multi_order_prepare_range(windows, node_lo: int, node_hi: int, p_lo: int, m_own: int):
    """Level 1 of the events whose source lies in ``[node_lo, node_hi)`` (pp_multiorder_prepare_range): ``windows`` from
    :func:`multi_order_node_loads`, ``p_lo = loads[0][node_lo]``, ``m_own = loads[0][node_hi] - p_lo > 0``.  Returns ``(level, tab)``: the
    rank's :class:`MultiOrderLevel` 1 (``row_ptr`` = the owned slice of layer 1's row pointers as offsets into the rank's own edges, ``col`` =
    ``tlast`` = global node ids; ``status`` bits 0 / 1 / 2 as pp_multiorder_prepare) and the continuation table of the WHOLE stream.  A node of
    the range with more than 4096 out-events sends the rank's events to the radix sort (second call); one read-back per call."""
    ei, weight, n, lift_ws = windows
    dev = ei.device
    m, n_own = ei.size(1), int(node_hi) - int(node_lo)
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        tab = torch.empty((m, 4), **i32)
        inst = torch.empty((m_own, 4), **i32)
        tptr, ibase = torch.empty(m_own + 1, **i32), torch.empty(m_own + 1, **i32)
        tlast, w = torch.empty(m_own, **i32), torch.empty(m_own, **f32)
        row_ptr = torch.empty(n_own + 1, **i32)
        ws = _workspace(L.pp_multiorder_prepare_range_ws_bytes(m, m_own), dev)
        for radix in ((True,) if m_own > 1024 * n_own else (False, True)):
            check(L.pp_multiorder_prepare_range(_p(ei), m, n, _p(weight), _p(lift_ws), lift_ws.numel(), int(node_lo), int(node_hi), int(p_lo), int(m_own),
                                                1 if radix else 0, _p(tab), _p(inst), _p(tptr), _p(ibase), _p(tlast), _p(w), _p(row_ptr), _p(ws), ws.numel(),
                                                _stream()), "pp_multiorder_prepare_range")
            types, status, children, _ = ws[:32].view(torch.int64).tolist()
            if not status & 16:
                break
    return MultiOrderLevel(types=types, children=children, status=status & ~16, tptr=tptr, ibase=ibase, inst=inst, row_ptr=row_ptr, col=tlast,
                           weight=w, tlast=tlast), tab


def multi_order_stitch(gathered: torch.Tensor, stride: int, last_at: int, row_lo: list[int], edge_lo: list[int]):
    """``(cand_ptr int32 [rows + 1], cand_last int32 [edges])`` of the next step from the all-gathered per-rank pieces, one launch
    (pp_multiorder_stitch): ``gathered`` int32 [world * stride], block r = rank r's row pointers (offsets into its own edges) and, from entry
    ``last_at`` on, the last nodes of its edges; ``row_lo`` / ``edge_lo`` [world + 1]: first global row / edge of every rank."""
    dev = require_device(gathered)
    world = len(row_lo) - 1
    if gathered.dtype != torch.int32 or gathered.numel() < world * stride:
        raise ValueError("multi_order_stitch: `gathered` must hold world * stride int32")
    gathered = gathered.contiguous()
    with torch.cuda.device(dev):
        cand_ptr = torch.empty(int(row_lo[-1]) + 1, dtype=torch.int32, device=dev)
        cand_last = torch.empty(int(edge_lo[-1]), dtype=torch.int32, device=dev)
        rows = (ctypes.c_int64 * (world + 1))(*[int(v) for v in row_lo])
        edges = (ctypes.c_int64 * (world + 1))(*[int(v) for v in edge_lo])
        check(lib().pp_multiorder_stitch(_p(gathered), int(stride), int(last_at), world, rows, edges, _p(cand_ptr), _p(cand_last), _stream()),
              "pp_multiorder_stitch")
    return cand_ptr, cand_last


class DeBruijn2Part:
    """Count phase of the order-2 builder on ONE RANK's node range (:func:`debruijn2_part_count`): sizes on the host, everything else on
    the device until :func:`debruijn2_part_fill`."""

    __slots__ = ("m", "n", "lo", "n_own", "world", "args", "ws", "bufs", "u2", "status", "a2", "e2", "a1", "n_halo", "n_send", "recv_counts", "send_counts",
                 "row_of", "send_slot", "ho_deg", "succ", "bip", "pad_rows")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def debruijn2_part_count(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int, node_lo: int, node_hi: int, cuts_dev: torch.Tensor,
                         rank: int, delta, weight: torch.Tensor | None = None, pad_rows: int | None = None) -> "DeBruijn2Part | None":
    """The order-2 builder for the rank that owns the nodes ``[node_lo, node_hi)`` of a partitioned stream: ``edge_index`` / ``time`` hold the
    (time-sorted) events that start or end in that range.  Everything :func:`debruijn2` counts, restricted to the owned middle nodes, plus the
    halo numbering (sources (a, b) with a foreign a, in (owner of a, b, a) order behind the owned rows) and the LOCAL ROW ORDER: owned rows (b, c)
    whose c another rank owns come first, grouped by that rank, ordered by (c, b) = the receiver's halo order — the send list of every exchange
    is the prefix ``[0, n_send)`` of a row matrix; ``row_of[local row]`` = lexicographic row.  ONE read-back.  ``None``: inputs the builder does
    not take — a shard without events or without nodes, a weight that is not float32 (the caller reports it in its agreement collective and
    every rank falls back).  Bad input is NOT raised here: a rank sees only its own events, so the caller gathers ``status`` (bit 0: node index
    out of range, bit 1: events not sorted by time, bit 2: a node with more than 64 in- / out-events) from all ranks and raises everywhere
    (a rank-local raise in front of a collective leaves the other ranks blocked in it)."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, time, weight, cuts_dev)
    stream = _event_stream(ei, time, weight)
    m, n = ei.size(1), int(num_nodes)
    world = int(cuts_dev.numel()) - 1
    n_own = int(node_hi) - int(node_lo)
    if stream is None or m == 0 or n_own <= 0:      # (pp_debruijn2_part_count leaves the shard-level outputs of such a rank unwritten: ADVICE r4)
        return None
    time, weight = stream
    pad_rows = max(int(pad_rows) if pad_rows is not None else n, 1)          # rows per rank of the padded first-order layout (>= the largest range)
    kind, di, df = resolve_delta(time.dtype, delta)
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        cap = max(m, 1)
        ws = _workspace(L.pp_debruijn2_ws_bytes(m, n), dev)
        bufs = {"fo_bwd_ptr": torch.empty(n_own + 1, **i32), "fo_fwd_ptr": torch.empty(n_own + 1, **i32), "fo_bwd_idx": torch.empty(cap, **i32),
                "fo_w": torch.empty(cap, **f32), "ho_fwd_ptr": torch.empty(cap + 1, **i32), "ho_bwd_ptr": torch.empty(cap + 1, **i32),
                "ho_deg": torch.empty(cap, **f32), "fo_deg": torch.empty(max(n, 1), **f32), "row_of": torch.empty(cap, **i32),
                "send_slot": torch.empty(cap, **i32), "fo_shard_bwd_ptr": torch.empty(n + 1, **i32),
                "bip_fwd_ptr": torch.empty(world * pad_rows + 1, **i32), "bip_fwd_idx": torch.empty(cap, **i32), "bip_bwd_ptr": torch.empty(cap + 1, **i32),
                "bip_bwd_idx": torch.empty(cap, **i32), "bip_self": torch.empty(world * pad_rows, **f32)}
        tcode = _DTYPE_CODE[time.dtype]
        check(L.pp_debruijn2_part_count(_p(ei), _p(time), tcode, m, n, int(node_lo), n_own, _p(cuts_dev), world, int(rank), kind, di, df, _p(weight),
                                        _p(bufs["fo_bwd_ptr"]), _p(bufs["fo_bwd_idx"]), _p(bufs["fo_w"]), _p(bufs["fo_fwd_ptr"]), _p(bufs["ho_fwd_ptr"]),
                                        _p(bufs["ho_bwd_ptr"]), _p(bufs["ho_deg"]), _p(bufs["fo_deg"]), _p(bufs["send_slot"]), _p(bufs["row_of"]), _p(bufs["fo_shard_bwd_ptr"]), pad_rows, _p(bufs["bip_fwd_ptr"]),
                                        _p(bufs["bip_fwd_idx"]), _p(bufs["bip_bwd_ptr"]), _p(bufs["bip_bwd_idx"]), _p(bufs["bip_self"]),
                                        _p(ws), ws.numel(), _stream()), "pp_debruijn2_part_count")
        head = ws[: 8 * (8 + 2 * (world + 1))].view(torch.int64).tolist()                 # the ONE read-back of this rank's graph construction
    u2, status, a2, e2, a1, n_halo, n_send = head[:7]
    if a2 >= _INT32_ROWS or u2 + n_halo >= _INT32_ROWS:          # int32 row pointers / local ids would wrap: reported like a hub node, every rank falls back
        status |= 4
    recv_ptr, send_ptr = head[8: 8 + world + 1], head[8 + world + 1: 8 + 2 * (world + 1)]
    return DeBruijn2Part(m=m, n=n, lo=int(node_lo), n_own=n_own, world=world, args=(tcode, kind, di, df, weight), ws=ws, bufs=bufs, u2=u2, status=status,
                         a2=a2, e2=e2, a1=a1, n_halo=n_halo, n_send=n_send, recv_counts=[recv_ptr[r + 1] - recv_ptr[r] for r in range(world)],
                         send_counts=[send_ptr[r + 1] - send_ptr[r] for r in range(world)], row_of=bufs["row_of"][:u2],
                         send_slot=bufs["send_slot"][:u2], ho_deg=bufs["ho_deg"], succ=bufs["fo_bwd_idx"][:u2], pad_rows=pad_rows,
                         bip=CsrPlan(n_dst=world * pad_rows, n_src=u2, fwd_ptr=bufs["bip_fwd_ptr"], fwd_idx=bufs["bip_fwd_idx"][:u2], fwd_val=None,
                                     bwd_ptr=bufs["bip_bwd_ptr"][: u2 + 1], bwd_idx=bufs["bip_bwd_idx"][:u2], bwd_val=None, self_coef=bufs["bip_self"]))


def debruijn2_part_fill(c: DeBruijn2Part):
    """Fill phase (after the weighted degrees of the halo rows arrived in ``c.ho_deg[u2: u2 + n_halo]`` and ``c.bufs["fo_deg"]`` holds the degrees of
    ALL first-order nodes): ``(ho CsrPlan over [owned | halo] sources, fo CsrPlan: destinations = owned nodes, sources = all nodes in the dense
    local order [owned | ids below lo | ids from hi on], order-2 nodes per owned first-order node)``."""
    dev = c.ws.device
    tcode, kind, di, df, weight = c.args
    b = c.bufs
    L = lib()
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        n_src = c.u2 + c.n_halo
        # source-major arrays with room for n_send entries in front: the AUGMENTED rows of the backward pass (see `aug` below) are
        # [one unit entry per sent row | the plain entries], i.e. the same arrays read from their start
        bwd_idx_all, bwd_val_all = torch.empty(c.n_send + c.a2, **i32), torch.empty(c.n_send + c.a2, **f32)
        ho = CsrPlan(n_dst=c.u2, n_src=n_src, fwd_ptr=b["ho_fwd_ptr"][: c.u2 + 1], fwd_idx=torch.empty(c.a2, **i32), fwd_val=torch.empty(c.a2, **f32),
                     bwd_ptr=b["ho_bwd_ptr"][: n_src + 1], bwd_idx=bwd_idx_all[c.n_send:], bwd_val=bwd_val_all[c.n_send:],
                     self_coef=torch.empty(c.u2, **f32))
        fo = CsrPlan(n_dst=c.n_own, n_src=c.n, fwd_ptr=b["fo_fwd_ptr"], fwd_idx=torch.empty(c.a1, **i32), fwd_val=torch.empty(c.a1, **f32),
                     bwd_ptr=b["fo_shard_bwd_ptr"], bwd_idx=torch.empty(c.a1, **i32), bwd_val=torch.empty(c.a1, **f32),
                     self_coef=torch.empty(c.n_own, **f32))
        if c.m > 0 and c.n_own > 0:
            check(L.pp_debruijn2_part_fill(tcode, c.m, c.n, c.lo, c.n_own, kind, di, df, _p(weight), _p(b["fo_bwd_ptr"]), _p(b["fo_fwd_ptr"]),
                                           _p(b["ho_fwd_ptr"]), _p(b["ho_bwd_ptr"]), _p(b["ho_deg"]), _p(b["fo_deg"]), c.a2, _p(ho.fwd_idx), _p(ho.fwd_val),
                                           _p(ho.bwd_idx), _p(ho.bwd_val), _p(ho.self_coef), _p(fo.fwd_idx), _p(fo.fwd_val), _p(fo.self_coef),
                                           _p(b["fo_shard_bwd_ptr"]), _p(fo.bwd_idx), _p(fo.bwd_val), _p(torch.empty(2 * c.a2, **i32)), _p(c.ws),
                                           c.ws.numel(), _stream()), "pp_debruijn2_part_fill")
        indeg = (b["fo_fwd_ptr"][1:] - b["fo_fwd_ptr"][:-1]).to(torch.float32)
        # Augmented source-major rows of the OWNED rows for the backward pass: a sent row (local id k < n_send) has no local out-edge — its
        # out-edges live on the rank that owns its head node, whose partial sum comes back as row k of the returned halo sums.  With those
        # stored behind dpre ([dpre | recv]) the returned sum is ONE more CSR entry (n_own + k, 1.0) of row k, and the fused backward kernels
        # (pp_gcn_backward_f32 / pp_gcn_input_grad_f32) do the fold, the self term, both products and the weight gradient in one pass.
        torch.arange(c.u2, c.u2 + c.n_send, out=bwd_idx_all[: c.n_send])
        bwd_val_all[: c.n_send] = 1.0
        aug_ptr = b["ho_bwd_ptr"][: c.u2 + 1] + torch.arange(c.u2 + 1, **i32).clamp_(max=c.n_send)
        ho.aug = (aug_ptr, bwd_idx_all, bwd_val_all)
    return ho, fo, indeg


def spmm(ptr, idx, val, n_rows: int, x: torch.Tensor, self_coef=None, s=None, bias=None, act: bool = False,
         heavy: HeavyRows | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Y[r] = act(sum_p val[p] * x[idx[p]] + self_coef[r] * s[r] + bias) — fp32, rows of width F.  ``heavy``: the hub rows of this
    CSR (``plan.fwd_heavy`` / ``plan.bwd_heavy``), summed by the chunked pre-pass."""
    dev = require_device(x, s, bias)
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise TypeError("DBGNN kernels are fp32")
    f = x.size(1)
    if f > 256:          # the row kernels own at most 64 lanes x 4 columns per row: wider matrices go through in 256-column blocks
        blocks = [spmm(ptr, idx, val, n_rows, x[:, c: c + 256], self_coef, None if s is None else s[:, c: c + 256],
                       None if bias is None else bias[c: c + 256], act, heavy) for c in range(0, f, 256)]
        y = torch.cat(blocks, dim=1)
        return y if out is None else out.copy_(y)
    if s is not None:
        s = s.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    slot, sums = _heavy_args(heavy, idx, val, x)
    with torch.cuda.device(dev):
        y = torch.empty((n_rows, f), dtype=torch.float32, device=dev) if out is None else out
        if out is not None and (tuple(out.shape) != (n_rows, f) or out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError("spmm: out must be a contiguous fp32 [n_rows, F] tensor")
        check(lib().pp_spmm_f32(_p(ptr), _p(idx), _p(val), n_rows, _p(x), f, _p(self_coef), _p(s), _p(bias), 1 if act else 0,
                                _p(slot), _p(sums), _p(y), _stream()), "pp_spmm_f32")
    return y


def bip_combine(a: torch.Tensor, p: torch.Tensor, deg: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """``ELU(a + deg[:, None] * (p + bias))`` in one pass (pp_bip_combine_f32)."""
    dev = require_device(a, p, deg, bias)
    a, p, deg = a.contiguous(), p.contiguous(), deg.to(torch.float32).contiguous()
    if a.dtype != torch.float32 or p.shape != a.shape or deg.numel() != a.size(0):
        raise ValueError("bip_combine: a, p [n, F] fp32 and deg [n] expected")
    with torch.cuda.device(dev):
        y = torch.empty_like(a)
        check(lib().pp_bip_combine_f32(_p(a), _p(p), _p(deg), _p(None if bias is None else bias.contiguous()), a.size(0), a.size(1), _p(y), _stream()),
              "pp_bip_combine_f32")
    return y


def bip_combine_backward(dy: torch.Tensor, y: torch.Tensor, deg: torch.Tensor, want_bias: bool):
    """Backward of :func:`bip_combine`: ``(d_a, d_p, d_bias or None)`` in one pass (pp_bip_combine_backward_f32)."""
    dev = require_device(dy, y, deg)
    dy, deg = dy.contiguous(), deg.to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        da, dp = torch.empty_like(y), torch.empty_like(y)
        db = torch.empty(y.size(1), dtype=torch.float32, device=dev) if want_bias else None
        check(lib().pp_bip_combine_backward_f32(_p(dy), _p(y), _p(deg), y.size(0), y.size(1), _p(da), _p(dp), _p(db), _stream()),
              "pp_bip_combine_backward_f32")
    return da, dp, db


def act_backward(dy: torch.Tensor, y: torch.Tensor | None, act: bool, want_dpre: bool = True, want_dbias: bool = False):
    dev = require_device(dy, y)
    dy = dy.contiguous()
    n, f = dy.shape
    with torch.cuda.device(dev):
        dpre = torch.empty_like(dy) if want_dpre else None
        dbias = torch.empty(f, dtype=torch.float32, device=dev) if want_dbias else None
        check(lib().pp_act_backward_f32(_p(dy), _p(y), n, f, 1 if act else 0, _p(dpre), _p(dbias), _stream()), "pp_act_backward_f32")
    return dpre, dbias


def dropout(x: torch.Tensor, p: float, seed: int, tag: int, row0: int = 0, rows: torch.Tensor | None = None, out: torch.Tensor | None = None):
    """Training-mode dropout with counter-based masks (see pp_dropout_f32): ``x * keep / (1 - p)``; ``out`` may be ``x`` itself."""
    dev = require_device(x, rows)
    x = x.contiguous()
    n, f = x.shape
    if rows is not None:
        rows = rows.to(torch.int64).contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(x)
        check(lib().pp_dropout_f32(_p(x), n, f, float(p), int(seed), int(tag), int(row0), _p(rows), _p(out), _stream()), "pp_dropout_f32")
    return out


def dropout_diag_rows(x: torch.Tensor, n: int, p: float, seed: int, tag: int, row0: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """``x[r] * d[row0 + r]`` with ``d[g]`` the factor :func:`dropout` gives element ``(g, g)`` of an ``[n, n]`` matrix — what dropout of an
    identity matrix leaves of ``I @ x`` (pp_dropout_diag_rows_f32); ``out`` may be ``x`` itself."""
    dev = require_device(x)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("dropout_diag_rows: a contiguous fp32 [n_rows, F] matrix expected")
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty_like(x)
        elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
            raise ValueError("dropout_diag_rows: out must be a contiguous fp32 tensor of x's shape on x's device")
        if x.size(1) > 0:
            check(lib().pp_dropout_diag_rows_f32(_p(x), x.size(0), x.size(1), int(n), float(p), int(seed), int(tag), int(row0), _p(out), _stream()),
                  "pp_dropout_diag_rows_f32")
    return out


def spmm_diag_drop_supported(f: int, heavy: HeavyRows | None) -> bool:
    """Whether :func:`spmm_diag_drop` takes rows of width ``f`` over a CSR with these hub rows (none: the chunked pre-pass sums unscaled rows)."""
    return f % 4 == 0 and 4 <= f <= 256 and (heavy is None or heavy.n_heavy == 0)


def spmm_diag_drop(ptr, idx, val, n_rows: int, x: torch.Tensor, self_coef, bias, act: bool, where: int, n: int, p: float, seed: int,
                   tag: int) -> torch.Tensor:
    """:func:`spmm` with ``s = x`` and the dropout factors ``d`` of an ``[n, n]`` identity's diagonal inside the kernel (pp_spmm_diag_drop_f32):
    ``where = 1`` scales every source row (``act(A diag(d) x + self_coef * d * x + bias)``), ``where = 2`` every output row."""
    dev = require_device(x, bias)
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise TypeError("DBGNN kernels are fp32")
    if where == 1 and x.size(0) < n:
        raise ValueError("spmm_diag_drop: the source matrix must have the identity's n rows")
    if bias is not None:
        bias = bias.contiguous()
    with torch.cuda.device(dev):
        y = torch.empty((n_rows, x.size(1)), dtype=torch.float32, device=dev)
        check(lib().pp_spmm_diag_drop_f32(_p(ptr), _p(idx), _p(val), n_rows, _p(x), x.size(1), _p(self_coef), _p(bias), 1 if act else 0, int(where),
                                          int(n), float(p), int(seed), int(tag), _p(y), _stream()), "pp_spmm_diag_drop_f32")
    return y


def _check_row_map(row_map: torch.Tensor, n: int) -> None:
    """A row map addresses the replicated ``[n, F]`` matrix inside the kernel: its range is verified ONCE per tensor (and in-place version) —
    one tiny reduction and a 16-byte read at the first use, nothing per step."""
    key = (row_map._version, int(n))
    if getattr(row_map, "_pp_map_range", None) == key:
        return
    if row_map.numel():
        lo, hi = minmax(row_map)
        if lo < 0 or hi >= n:
            raise IndexError(f"spmm_diag_drop_map: the row map holds ids outside [0, {n}) ({lo} .. {hi})")
    try:
        row_map._pp_map_range = key
    except Exception:
        pass


def spmm_diag_drop_map(ptr, idx, val, n_rows: int, x: torch.Tensor, self_coef, bias, act: bool, where: int, row_map: torch.Tensor, n: int,
                       p: float, seed: int, tag: int, n_self: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`spmm_diag_drop` on one rank's rectangular share of the graph (pp_spmm_diag_drop_map_f32): the CSR runs over local slots and
    ``row_map`` (int64, distinct global ids in ``[0, n)``, one per local source slot) says which row of the replicated ``[n, F]`` matrix a slot is.
    ``where = 1``: ``x = W^T [n, F]``, result ``[n_rows, F]`` (``out``: written there); ``where = 2``: ``x = dpre [n_self, F]`` over the transposed
    CSR of the ``n_rows`` source slots, result = the rank's partial ``dW^T [n, F]`` (rows no slot maps to are zero)."""
    dev = require_device(x, bias, row_map)
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise TypeError("DBGNN kernels are fp32")
    if row_map.dtype != torch.int64 or row_map.dim() != 1 or not row_map.is_contiguous():
        raise ValueError("spmm_diag_drop_map: the row map must be a contiguous int64 vector")
    n_self = n_rows if n_self is None else int(n_self)
    if where == 1 and (x.size(0) != n or row_map.numel() < n_rows):
        raise ValueError("spmm_diag_drop_map: where 1 needs the [n, F] matrix and a map entry for every local source slot")
    if where == 2 and (x.size(0) != n_self or row_map.numel() != n_rows):
        raise ValueError("spmm_diag_drop_map: where 2 needs dpre on the n_self owned rows and one map entry per source slot")
    _check_row_map(row_map, n)
    if bias is not None:
        bias = bias.contiguous()
    with torch.cuda.device(dev):
        if where == 2:
            y = torch.zeros((n, x.size(1)), dtype=torch.float32, device=dev)
        elif out is not None:
            if tuple(out.shape) != (n_rows, x.size(1)) or out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError("spmm_diag_drop_map: out must be a contiguous fp32 [n_rows, F] tensor")
            y = out
        else:
            y = torch.empty((n_rows, x.size(1)), dtype=torch.float32, device=dev)
        check(lib().pp_spmm_diag_drop_map_f32(_p(ptr), _p(idx), _p(val), n_rows, n_self, _p(x), x.size(1), _p(self_coef), _p(bias), 1 if act else 0,
                                              int(where), _p(row_map), int(n), float(p), int(seed), int(tag), _p(y), _stream()),
              "pp_spmm_diag_drop_map_f32")
    return y


def dropout_act_backward(dy: torch.Tensor, y_dropped: torch.Tensor | None, p: float, seed: int, tag: int, row0: int = 0,
                         rows: torch.Tensor | None = None, act: bool = True, want_dbias: bool = False):
    """``(dpre, dbias or None)``: backward of :func:`dropout` fused with the ELU backward of the activation underneath (``act``)."""
    dev = require_device(dy, y_dropped, rows)
    dy = dy.contiguous()
    n, f = dy.shape
    if y_dropped is not None:
        y_dropped = y_dropped.contiguous()
    if rows is not None:
        rows = rows.to(torch.int64).contiguous()
    with torch.cuda.device(dev):
        dpre = torch.empty_like(dy)
        dbias = torch.empty(f, dtype=torch.float32, device=dev) if want_dbias else None
        check(lib().pp_dropout_act_backward_f32(_p(dy), _p(y_dropped), n, f, float(p), int(seed), int(tag), int(row0), _p(rows), 1 if act else 0,
                                                _p(dpre), _p(dbias), _stream()), "pp_dropout_act_backward_f32")
    return dpre, dbias


def halo_fold(own: torch.Tensor, recv: torch.Tensor | None = None, slot: torch.Tensor | None = None, extra: torch.Tensor | None = None,
              self_coef: torch.Tensor | None = None, dpre: torch.Tensor | None = None, inplace: bool = True) -> torch.Tensor:
    """``own + recv[slot] (where slot >= 0) + extra + self_coef[:, None] * dpre`` in one pass (pp_halo_fold_f32); written into ``own`` when
    ``inplace``.  ``slot`` int32 [n]; fp32 matrices of one width (a multiple of 4)."""
    dev = require_device(own, recv, slot, extra, self_coef, dpre)
    if not own.is_contiguous():
        raise ValueError("halo_fold: own must be contiguous")
    if own.numel() == 0:
        return own if inplace else own.clone()
    if recv is not None and (slot is None or recv.size(0) == 0):
        recv = slot = None
    if slot is not None and recv is None:
        slot = None
    recv = None if recv is None else recv.contiguous()
    extra = None if extra is None else extra.contiguous()
    dpre = None if dpre is None else dpre.contiguous()
    if slot is not None and slot.dtype != torch.int32:
        raise TypeError("halo_fold: slot must be int32")
    with torch.cuda.device(dev):
        out = own if inplace else torch.empty_like(own)
        check(lib().pp_halo_fold_f32(_p(own), _p(recv), _p(slot), _p(extra), _p(self_coef), _p(dpre), own.size(0), own.size(1), _p(out), _stream()),
              "pp_halo_fold_f32")
    return out


def gather_rows(x: torch.Tensor, rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``x[rows]`` for an fp32 matrix whose width is a multiple of 4 (pp_spmm_f32 with one unit entry per output row)."""
    rows32 = rows.to(torch.int32).contiguous()
    n = int(rows32.numel())
    ptr = torch.arange(n + 1, dtype=torch.int32, device=rows32.device)
    return spmm(ptr, rows32, None, n, x, out=out)


def scale_rows(x: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    dev = require_device(x, coef)
    x = x.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty_like(x)
        check(lib().pp_scale_rows_f32(_p(x), _p(coef), x.size(0), x.size(1), _p(out), _stream()), "pp_scale_rows_f32")
    return out


def weight_grad(dy: torch.Tensor, x: torch.Tensor, want_bias: bool):
    """(dW [M,K], db [M] or None) of y = x W^T (+ b) from dy [N,M] and x [N,K] — MFMA kernel, fp32."""
    dev = require_device(dy, x)
    dy, x = dy.contiguous(), x.contiguous()
    n, m = dy.shape
    k = x.size(1)
    L = lib()
    with torch.cuda.device(dev):
        dw = torch.empty((m, k), dtype=torch.float32, device=dev)
        db = torch.empty(m, dtype=torch.float32, device=dev) if want_bias else None
        ws = _workspace(L.pp_weight_grad_ws_bytes(n, m, k), dev)
        check(L.pp_weight_grad_f32(_p(dy), _p(x), n, m, k, _p(dw), _p(db), _p(ws), ws.numel(), _stream()), "pp_weight_grad_f32")
    return dw, db


def dense_supported(p: int, q: int) -> int:
    """0: no HIP kernel for this layer shape (library GEMM); 1: widths 16/32/64 (also :func:`dense_backward`); 2: other widths whose
    zero-padded product fits the register-resident kernel (anything up to 64 x 64, 256 x 8, 8 x 256, ...); 3: 64/128/256 with a side > 64 (weights streamed through LDS)."""
    return int(lib().pp_dense_supported(int(p), int(q)))


def dense(a: torch.Tensor, weight: torch.Tensor, transposed: bool, bias: torch.Tensor | None = None,
          grad_act: torch.Tensor | None = None, want_colsum: bool = False):
    """``out = (a @ (weight.T if transposed else weight) + bias) * elu'`` on the matrix cores (fp32) where ``elu'`` is the ELU
    derivative recovered from the stored activation ``grad_act`` (``y > 0 ? 1 : y + 1``); returns ``(out, colsum or None)``.
    Shapes must satisfy :func:`dense_supported`."""
    dev = require_device(a, weight, bias, grad_act)
    a, weight = a.contiguous(), weight.contiguous()
    n, p = a.shape
    q = weight.size(0) if transposed else weight.size(1)
    if (weight.size(1) if transposed else weight.size(0)) != p:
        raise ValueError("dense: inner dimensions do not match")
    if bias is not None:
        bias = bias.contiguous()
    if grad_act is not None:
        grad_act = grad_act.contiguous()
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty((n, q), dtype=torch.float32, device=dev)
        colsum = torch.empty(q, dtype=torch.float32, device=dev) if want_colsum else None
        ws = _workspace(L.pp_wide_layer_ws_bytes(p, q), dev) if L.pp_dense_supported(p, q) == 3 else None       # (chunk-major / transposed W)
        check(L.pp_dense_f32(_p(a), _p(weight), 1 if transposed else 0, n, p, q, _p(bias), _p(grad_act), _p(colsum), _p(out), _p(ws),
                             0 if ws is None else ws.numel(), _stream()), "pp_dense_f32")
    return out, colsum


def spmm_act_backward(ptr, idx, val, n_rows: int, d: torch.Tensor, z: torch.Tensor, want_colsum: bool, drop: tuple | None = None,
                      out: torch.Tensor | None = None):
    """``dx = (A d) * elu'(z)`` with ``elu'`` from the stored activation ``z`` (``z > 0 ? 1 : z + 1``) and, optionally, the
    column sums of ``dx`` — one pass.  ``drop = (p, seed, tag, row0)``: ``z`` is stored dropped; mask and ``1 / (1 - p)`` go into ``dx``."""
    dev = require_device(d, z)
    dp, dseed, dtag, drow0 = _drop_args(drop)
    d, z = d.contiguous(), z.contiguous()
    f = d.size(1)
    with torch.cuda.device(dev):
        dx = torch.empty((n_rows, f), dtype=torch.float32, device=dev) if out is None else out
        if out is not None and (tuple(out.shape) != (n_rows, f) or out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError("spmm_act_backward: out must be a contiguous fp32 [n_rows, F] tensor")
        colsum = torch.empty(f, dtype=torch.float32, device=dev) if want_colsum else None
        check(lib().pp_spmm_act_backward_drop_f32(_p(ptr), _p(idx), _p(val), n_rows, _p(d), f, _p(z), _p(colsum), _p(dx), dp, dseed, dtag, drow0,
                                                  _stream()), "pp_spmm_act_backward_drop_f32")
    return dx, colsum


def _drop_args(drop):
    if drop is None:
        return 0.0, 0, 0, 0
    p, seed, tag, row0 = drop
    return float(p), int(seed), int(tag), int(row0)


def gcn_drop_supported(p: int, q: int) -> bool:
    """Layer shapes whose fused kernels take the ``drop`` argument (16/32/64 and the 128-wide shapes)."""
    return bool(lib().pp_gcn_drop_supported(int(p), int(q)))


def gcn_forward(ptr: torch.Tensor, idx: torch.Tensor, val: torch.Tensor | None, n_rows: int, x: torch.Tensor,
                self_coef: torch.Tensor | None, weight: torch.Tensor, bias: torch.Tensor | None, act: bool, want_agg: bool = False,
                heavy: HeavyRows | None = None, out: torch.Tensor | None = None, drop: tuple | None = None):
    """``act((A x + diag(self_coef) x) @ weight.T + bias)`` in one kernel (aggregation fused with the MFMA product);
    ``want_agg``: returns ``(y, A x + diag(self_coef) x)``.  ``out``: a contiguous ``[n_rows, Q]`` fp32 tensor to write ``y`` into
    (e.g. the head of a buffer whose tail receives halo rows).  ``drop = (p, seed, tag, row0)``: training-mode dropout of ``y`` fused into
    the epilogue (counter-based mask of :func:`dropout`; needs :func:`gcn_drop_supported`)."""
    dev = require_device(ptr, idx, val, x, self_coef, weight, bias)
    dp, dseed, dtag, drow0 = _drop_args(drop)
    x, weight = x.contiguous(), weight.contiguous()
    q, p = weight.shape
    if x.size(1) != p:
        raise ValueError("gcn_forward: inner dimensions do not match")
    if bias is not None:
        bias = bias.contiguous()
    with torch.cuda.device(dev):
        if out is None:
            y = torch.empty((n_rows, q), dtype=torch.float32, device=dev)
        else:
            if tuple(out.shape) != (n_rows, q) or out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError("gcn_forward: out must be a contiguous fp32 [n_rows, Q] tensor")
            y = out
        agg = torch.empty((n_rows, p), dtype=torch.float32, device=dev) if want_agg else None
        slot, sums = _heavy_args(heavy, idx, val, x)
        check(lib().pp_gcn_forward_drop_f32(_p(ptr), _p(idx), _p(val), n_rows, x.size(0), _p(x), p, _p(self_coef), _p(weight), q, _p(bias),
                                            1 if act else 0, _p(slot), _p(sums), _p(agg), _p(y), dp, dseed, dtag, drow0, _stream()),
              "pp_gcn_forward_drop_f32")
    return (y, agg) if want_agg else y


def gcn_backward(ptr, idx, val, n_rows: int, dpre: torch.Tensor, self_coef, x: torch.Tensor, weight: torch.Tensor, fuse_act: bool,
                 want_colsum: bool, heavy: HeavyRows | None = None, n_self: int | None = None, drop: tuple | None = None):
    """Backward of :func:`gcn_forward` in one kernel: ``(d_in, colsum_in or None, dW)`` from the gradient ``dpre`` w.r.t. the
    layer's pre-activation, over the SOURCE-major CSR (``ptr``/``idx``/``val`` = the plan's ``bwd_*`` arrays).
    ``n_self`` (default ``n_rows``): partition plans — ``n_rows`` = owned + halo source rows, ``dpre`` has the ``n_self`` owned rows.
    ``drop = (p, seed, tag, row0)`` (with ``fuse_act``): ``x`` is the DROPPED activation of the layer below; its mask and ``1 / (1 - p)`` go
    into ``d_in`` together with the ELU'."""
    dev = require_device(ptr, idx, val, dpre, self_coef, x, weight)
    dp, dseed, dtag, drow0 = _drop_args(drop)
    dpre, x, weight = dpre.contiguous(), x.contiguous(), weight.contiguous()
    m, k = weight.shape
    n_self = n_rows if n_self is None else int(n_self)
    # (dpre may hold MORE rows than n_self: an augmented CSR of a partition shard also gathers the returned halo sums stored behind the owned rows)
    if dpre.size(1) != m or x.size(1) != k or x.size(0) != n_rows or dpre.size(0) < n_self or n_self > n_rows:
        raise ValueError("gcn_backward: shapes do not match")
    L = lib()
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        d_in = torch.empty((n_rows, k), **f32)
        colsum = torch.empty(k, **f32) if want_colsum else None
        dw = torch.empty((m, k), **f32)
        slot, sums = _heavy_args(heavy, idx, val, dpre)
        ws = _workspace(L.pp_gcn_backward_ws_bytes(n_rows), dev)
        check(L.pp_gcn_backward_nnz_f32(_p(ptr), _p(idx), _p(val), n_rows, n_self, int(idx.numel()), _p(dpre), m, _p(self_coef), _p(x), k, _p(weight),
                                        1 if fuse_act else 0, _p(slot), _p(sums), _p(d_in), _p(colsum), _p(dw), _p(ws), ws.numel(), dp, dseed, dtag,
                                        drow0, _stream()), "pp_gcn_backward_nnz_f32")
    return d_in, colsum, dw


def gcn_backward_below(ptr, idx, val, n_rows: int, dpre: torch.Tensor, self_coef, x: torch.Tensor, weight: torch.Tensor, agg_below: torch.Tensor):
    """:func:`gcn_backward` of the second layer of a stack whose first layer takes no input gradient, with that layer's weight gradient
    formed in the same kernel: ``(colsum, dW, dW_below)`` where ``colsum`` = column sums of ``d_in = (G W) * ELU'(x)`` (the first layer's bias
    gradient) and ``dW_below = d_in^T agg_below`` (``agg_below`` = the ``A x`` kept by the first layer's :func:`gcn_forward`).  ``d_in`` is never
    stored.  64-wide layers on a whole graph without hub rows and without dropout only: anything else is a ValueError."""
    dev = require_device(ptr, idx, val, dpre, self_coef, x, weight, agg_below)
    dpre, x, weight, agg_below = dpre.contiguous(), x.contiguous(), weight.contiguous(), agg_below.contiguous()
    m, k = weight.shape
    if dpre.size(1) != m or x.size(1) != k or x.size(0) != n_rows or dpre.size(0) < n_rows or agg_below.size(0) != n_rows:
        raise ValueError("gcn_backward_below: shapes do not match")
    L = lib()
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        colsum = torch.empty(k, **f32)
        dw = torch.empty((m, k), **f32)
        dw_below = torch.empty((k, agg_below.size(1)), **f32)
        ws = _workspace(L.pp_gcn_backward_below_ws_bytes(n_rows), dev)
        check(L.pp_gcn_backward_below_f32(_p(ptr), _p(idx), _p(val), n_rows, n_rows, int(idx.numel()), _p(dpre), m, _p(self_coef), _p(x), k, _p(weight),
                                          1, None, None, None, _p(colsum), _p(dw), _p(ws), ws.numel(), 0.0, 0, 0, 0, _p(agg_below),
                                          agg_below.size(1), _p(dw_below), _stream()), "pp_gcn_backward_below_f32")
    return colsum, dw, dw_below


def gcn_fused_supported(p: int, q: int) -> int:
    """1: fused forward + one-kernel backward (widths 16/32/64); 2: fused forward + input-gradient kernel (128-wide shapes); 0: neither."""
    return int(lib().pp_gcn_fused_supported(int(p), int(q)))


def gcn_input_grad(ptr, idx, val, n_rows: int, dpre: torch.Tensor, self_coef, weight: torch.Tensor, x_act: torch.Tensor | None,
                   want_colsum: bool, heavy: HeavyRows | None = None, n_self: int | None = None, drop: tuple | None = None):
    """``((A^T dpre + diag(self_coef) dpre) @ weight) * elu'(x_act)`` (no activation factor when ``x_act`` is None) and optionally its
    column sums, over the SOURCE-major CSR — the input gradient of a 128-wide fused layer (``drop``: as in :func:`gcn_backward`)."""
    dev = require_device(ptr, idx, val, dpre, self_coef, weight, x_act)
    dp, dseed, dtag, drow0 = _drop_args(drop)
    dpre, weight = dpre.contiguous(), weight.contiguous()
    m, k = weight.shape
    n_self = n_rows if n_self is None else int(n_self)
    if dpre.size(1) != m or dpre.size(0) < n_self or n_self > n_rows or (x_act is not None and tuple(x_act.shape) != (n_rows, k)):
        raise ValueError("gcn_input_grad: shapes do not match")
    if x_act is not None:
        x_act = x_act.contiguous()
    L = lib()
    with torch.cuda.device(dev):
        d_in = torch.empty((n_rows, k), dtype=torch.float32, device=dev)
        colsum = torch.empty(k, dtype=torch.float32, device=dev) if want_colsum else None
        slot, sums = _heavy_args(heavy, idx, val, dpre)
        ws = _workspace(L.pp_wide_layer_ws_bytes(m, k), dev)              # (only the shapes with a side of 256 use it: W^T)
        check(L.pp_gcn_input_grad_drop_f32(_p(ptr), _p(idx), _p(val), n_rows, n_self, _p(dpre), m, _p(self_coef), _p(weight), k, _p(x_act),
                                           1 if x_act is not None else 0, _p(slot), _p(sums), _p(d_in), _p(colsum), _p(ws), ws.numel(), dp, dseed,
                                           dtag, drow0, _stream()), "pp_gcn_input_grad_drop_f32")
    return d_in, colsum


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, want_grad: bool = True):
    """(mean cross-entropy [scalar tensor], d loss / d logits or None) in one pass; logits [N, C<=64] fp32, target int64 [N]."""
    dev = require_device(logits, target)
    logits = logits.contiguous()
    target = target.to(torch.int64).contiguous()
    n, c = logits.shape
    with torch.cuda.device(dev):
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        grad = torch.empty_like(logits) if want_grad else None
        L = lib()
        ws = _workspace(L.pp_cross_entropy_ws_bytes(), dev)
        check(L.pp_cross_entropy_f32(_p(logits), _p(target), n, c, _p(loss), _p(grad), _p(ws), ws.numel(), _stream()), "pp_cross_entropy_f32")
    return loss[0], grad


class MaskedSums(NamedTuple):
    """The 32-byte device result of pp_cross_entropy_masked_f32, as two views of one buffer."""
    values: torch.Tensor      # float32 [4]: sum w[y] nll, sum w[y], their quotient (the mean loss), 1 / sum w[y] (0: nothing valid selected)
    counts: torch.Tensor      # int64 [2]: selected rows, selected rows whose target lies outside [0, C)


def _selection(what: str, n: int, c: int, target, mask, weight=None):
    target = target.contiguous()
    if target.dtype != torch.int64 or target.dim() != 1 or target.numel() != n:
        raise ValueError(f"{what}: target must be int64 [{n}]")
    if mask is not None:
        if mask.dtype != torch.bool or mask.dim() != 1 or mask.numel() != n:
            raise ValueError(f"{what}: mask must be bool [{n}]")
        mask = mask.contiguous()
    if weight is not None:
        if weight.dtype != torch.float32 or weight.dim() != 1 or weight.numel() != c:
            raise ValueError(f"{what}: weight must be float32 [{c}]")
        weight = weight.contiguous()
    return target, mask, weight


def cross_entropy_masked(logits: torch.Tensor, target: torch.Tensor, mask: torch.Tensor | None = None, weight: torch.Tensor | None = None,
                         ignore_index: int | None = None, want_grad: bool = True):
    """``(sums, raw_grad)`` of the class-weighted cross-entropy over the rows that ``mask`` (bool [N]; None: all) and ``ignore_index``
    (None: unused) select, in one pass and without a read-back: ``sums`` is a :class:`MaskedSums` on the device, ``raw_grad`` [N, C]
    (None without ``want_grad``) the gradient of the SUM reduction — ``w[y] (softmax - onehot)`` on selected rows, exact zeros elsewhere;
    the mean's gradient is ``raw_grad * sums.values[3]``.  logits [N, C<=64] fp32, target int64 [N], weight fp32 [C] or None."""
    dev = require_device(logits, target, mask, weight)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("cross_entropy_masked: logits must be float32 [N, C]")
    logits = logits.contiguous()
    n, c = logits.shape
    target, mask, weight = _selection("cross_entropy_masked", n, c, target, mask, weight)
    with torch.cuda.device(dev):
        result = torch.empty(4, dtype=torch.int64, device=dev)
        grad = torch.empty_like(logits) if want_grad else None
        L = lib()
        ws = _workspace(L.pp_cross_entropy_masked_ws_bytes(), dev)
        check(L.pp_cross_entropy_masked_f32(_p(logits), _p(target), _p(mask), _p(weight), n, c, 0 if ignore_index is None else int(ignore_index),
                                            0 if ignore_index is None else 1, _p(result), _p(grad), _p(ws), ws.numel(), _stream()),
              "pp_cross_entropy_masked_f32")
    return MaskedSums(result[:2].view(torch.float32), result[2:]), grad


class MaskedRawSums(NamedTuple):
    """The 32-byte device result of pp_cross_entropy_masked_sums_f32, as two views of one buffer."""
    sums: torch.Tensor        # float64 [2]: sum w[y] nll, sum w[y] — not yet rounded to fp32: a partitioned model adds its ranks' sums first
    counts: torch.Tensor      # int64 [2]: selected rows, selected rows whose target lies outside [0, C)


def cross_entropy_masked_sums(logits: torch.Tensor, target: torch.Tensor, mask: torch.Tensor | None = None, weight: torch.Tensor | None = None,
                              ignore_index: int | None = None, want_grad: bool = True):
    """:func:`cross_entropy_masked` for one rank of a partitioned model: ``(raw, raw_grad)`` with ``raw`` a :class:`MaskedRawSums` — the
    float64 sums as they stand before :func:`masked_finish` — and the same ``raw_grad``.  An empty ``[0, C]`` share gives zero sums."""
    dev = require_device(logits, target, mask, weight)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("cross_entropy_masked_sums: logits must be float32 [N, C]")
    logits = logits.contiguous()
    n, c = logits.shape
    target, mask, weight = _selection("cross_entropy_masked_sums", n, c, target, mask, weight)
    with torch.cuda.device(dev):
        result = torch.empty(4, dtype=torch.int64, device=dev)
        grad = torch.empty_like(logits) if want_grad else None
        L = lib()
        ws = _workspace(L.pp_cross_entropy_masked_ws_bytes(), dev)
        check(L.pp_cross_entropy_masked_sums_f32(_p(logits), _p(target), _p(mask), _p(weight), n, c, 0 if ignore_index is None else int(ignore_index),
                                                 0 if ignore_index is None else 1, _p(result), _p(grad), _p(ws), ws.numel(), _stream()),
              "pp_cross_entropy_masked_sums_f32")
    return MaskedRawSums(result[:2].view(torch.float64), result[2:]), grad


def masked_finish(sums: torch.Tensor, counts: torch.Tensor) -> MaskedSums:
    """float64 ``[2]`` sums and int64 ``[2]`` counts (a rank's, or the all-reduced ones) -> the :class:`MaskedSums` that
    :func:`cross_entropy_masked` returns for the same sums (pp_masked_finish_f32: the same arithmetic)."""
    dev = require_device(sums, counts)
    if sums.dtype != torch.float64 or counts.dtype != torch.int64 or sums.numel() != 2 or counts.numel() != 2:
        raise ValueError("masked_finish: float64 [2] sums and int64 [2] counts expected")
    sums, counts = sums.contiguous(), counts.contiguous()
    with torch.cuda.device(dev):
        result = torch.empty(4, dtype=torch.int64, device=dev)
        check(lib().pp_masked_finish_f32(_p(sums), _p(counts), _p(result), _stream()), "pp_masked_finish_f32")
    return MaskedSums(result[:2].view(torch.float32), result[2:])


def confusion(logits: torch.Tensor, target: torch.Tensor, mask: torch.Tensor | None = None, ignore_index: int | None = None,
              with_status: bool = False):
    """Confusion matrix int64 [C, C] (row = true class, column = predicted class) of ``argmax(logits, 1)`` over the selected rows — the
    selection of :func:`cross_entropy_masked`; the prediction is the lowest column holding the row maximum, a NaN counting as the maximum.
    ``with_status``: the flat int64 [C*C + 1] buffer instead, whose last word counts the selected rows skipped for a target outside
    [0, C) (one read-back gives both)."""
    dev = require_device(logits, target, mask)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("confusion: logits must be float32 [N, C]")
    logits = logits.contiguous()
    n, c = logits.shape
    target, mask, _ = _selection("confusion", n, c, target, mask)
    with torch.cuda.device(dev):
        buf = torch.empty(c * c + 1, dtype=torch.int64, device=dev)
        check(lib().pp_confusion_f32(_p(logits), _p(target), _p(mask), n, c, 0 if ignore_index is None else int(ignore_index),
                                     0 if ignore_index is None else 1, _p(buf), _p(buf[c * c:]), _stream()), "pp_confusion_f32")
    return buf if with_status else buf[: c * c].view(c, c)


def dense_backward(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, fuse_act: bool, want_input_grad: bool, want_colsum: bool,
                   want_bias: bool):
    """Backward of ``y = x @ weight.T (+ b)`` in one pass: ``(d_in or None, colsum_in or None, dW, db or None)`` with
    ``d_in = (dy @ weight) * elu'(x)`` when ``fuse_act``.  Shapes must satisfy :func:`dense_supported`."""
    dev = require_device(dy, x, weight)
    dy, x, weight = dy.contiguous(), x.contiguous(), weight.contiguous()
    n, m = dy.shape
    k = x.size(1)
    L = lib()
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        d_in = torch.empty((n, k), **f32) if want_input_grad else None
        colsum = torch.empty(k, **f32) if (want_input_grad and want_colsum) else None
        dw = torch.empty((m, k), **f32)
        db = torch.empty(m, **f32) if want_bias else None
        ws = _workspace(L.pp_dense_backward_ws_bytes(n), dev)
        check(L.pp_dense_backward_f32(_p(dy), _p(x), _p(weight), n, m, k, 1 if fuse_act else 0, _p(d_in), _p(colsum), _p(dw), _p(db),
                                      _p(ws), ws.numel(), _stream()), "pp_dense_backward_f32")
    return d_in, colsum, dw, db


def head_supported(ha: int, hx: int, hb: int, c: int) -> bool:
    """Whether the fused DBGNN head (:func:`head_forward` / :func:`head_backward`) takes these widths: ``agg`` [n, ha], ``x`` [n, hx],
    bipartite width ``hb`` (each 16, 32 or 64) and ``c`` <= 16 classes."""
    return bool(lib().pp_dbgnn_head_supported(ha, hx, hb, c))


def head_forward(agg: torch.Tensor, x: torch.Tensor, deg: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                 wlin: torch.Tensor, blin: torch.Tensor):
    """``z = ELU(agg @ w1.T + deg[:, None] * (x @ w2.T + b2 + b1))`` and ``logits = z @ wlin.T + blin`` in one kernel
    (pp_dbgnn_head_forward_f32): ``(z, logits)``.  Shapes must satisfy :func:`head_supported`."""
    dev = require_device(agg, x, deg, w1, b1, w2, b2, wlin, blin)
    agg, x, deg = agg.contiguous(), x.contiguous(), deg.to(torch.float32).contiguous()
    w1, b1, w2, b2, wlin, blin = (t.contiguous() for t in (w1, b1, w2, b2, wlin, blin))
    n, ha = agg.shape
    hx, hb, c = x.size(1), w1.size(0), wlin.size(0)
    if (agg.dtype != torch.float32 or x.dtype != torch.float32 or x.size(0) != n or deg.numel() != n or tuple(w1.shape) != (hb, ha)
            or tuple(w2.shape) != (hb, hx) or wlin.size(1) != hb or b1.numel() != hb or b2.numel() != hb or blin.numel() != c):
        raise ValueError("head_forward: agg [n, Ha], x [n, Hx], deg [n], w1 [Hb, Ha], w2 [Hb, Hx], wlin [C, Hb] (fp32) and their biases expected")
    with torch.cuda.device(dev):
        z = torch.empty((n, hb), dtype=torch.float32, device=dev)
        logits = torch.empty((n, c), dtype=torch.float32, device=dev)
        check(lib().pp_dbgnn_head_forward_f32(_p(agg), _p(x), _p(deg), _p(w1), _p(b1), _p(w2), _p(b2), _p(wlin), _p(blin), n, ha, hx, hb, c,
                                              _p(z), _p(logits), _stream()), "pp_dbgnn_head_forward_f32")
    return z, logits


def head_backward(dlogits: torch.Tensor, z: torch.Tensor, agg: torch.Tensor, x: torch.Tensor, deg: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
                  wlin: torch.Tensor, want_colsum: bool = True):
    """Backward of :func:`head_forward` (pp_dbgnn_head_backward_f32): ``(d_agg, dpre_fo, colsum_fo or None, dW1, dW2, db1, db2, dWlin, dblin)``
    with ``dpre_fo`` the gradient w.r.t. the PRE-activation behind ``x`` and ``colsum_fo`` its column sums (that layer's bias gradient)."""
    dev = require_device(dlogits, z, agg, x, deg, w1, w2, wlin)
    dlogits, z, agg, x, deg = dlogits.contiguous(), z.contiguous(), agg.contiguous(), x.contiguous(), deg.to(torch.float32).contiguous()
    w1, w2, wlin = w1.contiguous(), w2.contiguous(), wlin.contiguous()
    n, ha = agg.shape
    hx, hb, c = x.size(1), w1.size(0), wlin.size(0)
    if tuple(dlogits.shape) != (n, c) or tuple(z.shape) != (n, hb) or x.size(0) != n or deg.numel() != n or dlogits.dtype != torch.float32:
        raise ValueError("head_backward: dlogits [n, C], z [n, Hb], agg [n, Ha], x [n, Hx] (fp32) and deg [n] expected")
    L = lib()
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        d_agg, dpre_fo = torch.empty((n, ha), **f32), torch.empty((n, hx), **f32)
        colsum = torch.empty(hx, **f32) if want_colsum else None
        dw1, dw2, dwlin = torch.empty((hb, ha), **f32), torch.empty((hb, hx), **f32), torch.empty((c, hb), **f32)
        db1, db2, dblin = torch.empty(hb, **f32), torch.empty(hb, **f32), torch.empty(c, **f32)
        ws = _workspace(L.pp_dbgnn_head_backward_ws_bytes(n), dev)
        check(L.pp_dbgnn_head_backward_f32(_p(dlogits), _p(z), _p(agg), _p(x), _p(deg), _p(w1), _p(w2), _p(wlin), n, ha, hx, hb, c,
                                           _p(d_agg), _p(dpre_fo), _p(colsum), _p(dw1), _p(dw2), _p(db1), _p(db2), _p(dwlin), _p(dblin), _p(ws), ws.numel(), _stream()),
              "pp_dbgnn_head_backward_f32")
    return d_agg, dpre_fo, colsum, dw1, dw2, db1, db2, dwlin, dblin


# ------------------------------------------------------------------ order selection (csrc/pp_selection.hip)
_INDEX_WIDE = {torch.int32: 0, torch.int64: 1}


def _index_vector(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype not in _INDEX_WIDE:
        raise TypeError(f"{what}: int32 or int64 expected, got {t.dtype}")
    return t.reshape(-1).contiguous()


def walk_counts(row_ptr: torch.Tensor, col: torch.Tensor, n: int, K: int) -> tuple[list, list]:
    """``(totals, starts)`` as lists of Python ints for k = 1..K (pp_walk_counts_i64): ``totals[k - 1]`` the number of walks of length k of the
    graph with source-major CSR ``row_ptr`` [n + 1] / ``col`` (int32 or int64 each), ``starts[k - 1]`` the number of nodes that start one — the
    path counts of ``MultiOrderModel.get_mon_dof`` without a line-graph lift.  ``OverflowError`` when a count leaves int64 (the message names the
    first such order; the error carries the saturated ``totals`` and the exact ``starts``); ``IndexError`` for a column outside [0, n), ``ValueError`` for a malformed ``row_ptr``."""
    row_ptr, col = _index_vector(row_ptr, "walk_counts: row_ptr"), _index_vector(col, "walk_counts: col")
    dev = require_device(row_ptr, col)
    n, K = int(n), int(K)
    if K < 1 or row_ptr.numel() != n + 1:
        raise ValueError("walk_counts: K >= 1 and row_ptr of n + 1 entries expected")
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty(3 * K + 1, dtype=torch.int64, device=dev)
        ws = _workspace(L.pp_walk_counts_ws_bytes(n, col.numel(), K), dev)
        check(L.pp_walk_counts_i64(_p(row_ptr), _INDEX_WIDE[row_ptr.dtype], _p(col), _INDEX_WIDE[col.dtype], n, col.numel(), K, _p(out), _p(ws),
                                   ws.numel(), _stream()), "pp_walk_counts_i64")
        out = out.tolist()
    totals, starts, saturated, status = out[:K], out[K:2 * K], out[2 * K:3 * K], out[3 * K]
    _bad_index(status, "walk_counts")
    if status & 2:
        raise ValueError("walk_counts: row_ptr is not an ascending pointer array over col")
    if any(saturated):
        k = saturated.index(1) + 1
        error = OverflowError(f"walk_counts: the number of walks of length {k} does not fit int64")
        error.totals, error.starts = totals, starts          # (saturated totals read INT64_MAX; the starts are exact)
        raise error
    return totals, starts


def mon_layer_llh(row_ptr: torch.Tensor, weight: torch.Tensor, sel: torch.Tensor | None = None, freq: torch.Tensor | None = None) -> tuple[float, float]:
    """``(T, I)`` of one layer in float64 (pp_mon_layer_llh_f64): ``T = sum_e w_e log(w_e / S_row(e))`` over the layer's source-major CSR
    (``row_ptr`` int32 / int64, ``weight`` float32) and ``I = sum_s freq_s log(1 / outdegree(row of edge sel_s))`` for a selection of edge ids
    (int32 / int64) with float32 ``freq`` (``None``: I = 0.0).  Bit-reproducible, and the same for either integer width."""
    row_ptr = _index_vector(row_ptr, "mon_layer_llh: row_ptr")
    weight = weight.contiguous()
    if weight.dtype != torch.float32:
        raise TypeError("mon_layer_llh: float32 weights expected")
    n_sel = 0
    if sel is not None:
        sel, freq = _index_vector(sel, "mon_layer_llh: sel"), freq.contiguous()
        if freq.dtype != torch.float32 or freq.numel() != sel.numel():
            raise TypeError("mon_layer_llh: one float32 freq per selected edge expected")
        n_sel = sel.numel()
    dev = require_device(row_ptr, weight, sel, freq)
    n_rows, n_edges = row_ptr.numel() - 1, weight.numel()
    if n_rows < 0:
        raise ValueError("mon_layer_llh: empty row_ptr")
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty(3, dtype=torch.float64, device=dev)
        ws = _workspace(L.pp_mon_layer_llh_ws_bytes(n_rows, n_edges, n_sel), dev)
        check(L.pp_mon_layer_llh_f64(_p(row_ptr), _INDEX_WIDE[row_ptr.dtype], n_rows, _p(weight), n_edges, _p(sel),
                                     0 if sel is None else _INDEX_WIDE[sel.dtype], _p(freq), n_sel, _p(out), out.data_ptr() + 16, _p(ws), ws.numel(),
                                     _stream()), "pp_mon_layer_llh_f64")
        host = out.cpu()
    status = int(host[2:].view(torch.int64))
    _bad_index(status, "mon_layer_llh: selected edge")
    if status & 2:
        raise ValueError("mon_layer_llh: row_ptr is not an ascending pointer array over the weights")
    return float(host[0]), float(host[1])


def mon_zeroth_llh(node_sequence: torch.Tensor, dag_num_nodes: torch.Tensor, dag_weight: torch.Tensor, n: int):
    """``(Z, Z0)`` of a walk store in float64 (pp_mon_zeroth_llh_f64): the zeroth-order term of the walks' first nodes and the log-likelihood of
    the zeroth-order model.  ``None`` when the reference's formula is not the one the kernel computes — a node id of [0, n) that never occurs or
    one outside (``torch.unique``'s counts are then indexed by rank), walk lengths that do not fit the store: the caller takes the torch route."""
    seq = node_sequence.reshape(-1).contiguous()
    lengths, weight = dag_num_nodes.contiguous(), dag_weight.contiguous()
    dev = require_device(seq, lengths, weight)
    if seq.dtype != torch.int64 or lengths.dtype != torch.int64 or weight.dtype != torch.float32:
        raise TypeError("mon_zeroth_llh: node_sequence / dag_num_nodes int64 and dag_weight float32 expected")
    positions, walks, n = seq.numel(), lengths.numel(), int(n)
    if positions == 0 or walks == 0 or n <= 0 or weight.numel() != walks or positions >= _INT32_ROWS or n >= _INT32_ROWS:
        return None
    L = lib()
    with torch.cuda.device(dev):
        out = torch.empty(3, dtype=torch.float64, device=dev)
        ws = _workspace(L.pp_mon_zeroth_llh_ws_bytes(positions, walks, n), dev)
        check(L.pp_mon_zeroth_llh_f64(_p(seq), positions, _p(lengths), _p(weight), walks, n, _p(out), out.data_ptr() + 16, _p(ws), ws.numel(),
                                      _stream()), "pp_mon_zeroth_llh_f64")
        host = out.cpu()
    if int(host[2:].view(torch.int64)) != 0:
        return None
    return float(host[0]), float(host[1])


# ------------------------------------------------------------------ rolling time windows (csrc/pp_rolling.hip)
ROLLING_BAD_INDEX, ROLLING_BAD_ORDER, ROLLING_LONG_RUN = 1, 2, 4       # status bits of rolling_count's report


def rolling_key_dtype(num_nodes: int) -> torch.dtype:
    """dtype of the ``src << bits | dst`` keys of a graph of ``num_nodes`` nodes: int32 while both indices fit 16 bits, int64 beyond."""
    return torch.int32 if 2 * max(int(max(num_nodes, 2) - 1).bit_length(), 1) <= 32 else torch.int64


def rolling_group(edge_index: torch.Tensor, time: torch.Tensor, num_nodes: int):
    """``(keys, perm, flags)`` of a time-sorted stream (pp_rolling_group): the pair keys ascending, the event at every position (stable, so
    a pair's events are one run in time order) and the flag word [1] (bit 0 an index outside [0, num_nodes), bit 1 not time-sorted or a NaN),
    which stays on the device: :func:`rolling_count` hands it back with its report."""
    ei = _edge_index(edge_index)
    dev = require_device(ei, time)
    time, _ = _event_stream(ei, time)
    m, num_nodes = ei.size(1), int(num_nodes)
    L = lib()
    with torch.cuda.device(dev):
        keys = torch.empty(m, dtype=rolling_key_dtype(num_nodes), device=dev)
        perm = torch.empty(m, dtype=torch.int32, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(L.pp_rolling_group_ws_bytes(m, num_nodes), dev)
        check(L.pp_rolling_group(_p(ei), _p(time), _DTYPE_CODE[time.dtype], m, num_nodes, _p(keys), _p(perm), _p(flags), _p(ws), ws.numel(),
                                 _stream()), "pp_rolling_group")
    return keys, perm, flags


def rolling_bounds(time: torch.Tensor, starts: torch.Tensor, ends: torch.Tensor):
    """``(lo, hi)`` int32 [W]: the first event with ``time >= starts[w]`` / ``>= ends[w]`` of a sorted int64 or float64 ``time``
    (pp_rolling_bounds); ``starts`` / ``ends`` in the dtype of ``time``, non-decreasing."""
    dev = require_device(time, starts, ends)
    if time.dtype not in (torch.int64, torch.float64) or starts.dtype != time.dtype or ends.dtype != time.dtype:
        raise TypeError("rolling_bounds: time, starts and ends must share the dtype int64 or float64")
    time, starts, ends = time.contiguous(), starts.contiguous(), ends.contiguous()
    W = starts.numel()
    if ends.numel() != W:
        raise ValueError("rolling_bounds: one start and one end per window")
    with torch.cuda.device(dev):
        lo = torch.empty(W, dtype=torch.int32, device=dev)
        hi = torch.empty(W, dtype=torch.int32, device=dev)
        check(lib().pp_rolling_bounds(_p(time), _DTYPE_CODE[time.dtype], time.numel(), _p(starts), _p(ends), W, _p(lo), _p(hi), _stream()),
              "pp_rolling_bounds")
    return lo, hi


def rolling_count(keys: torch.Tensor, perm: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, w0: int, w1: int, max_run: int,
                  flags: torch.Tensor):
    """``(cnt, report)`` for the windows ``w0 .. w1 - 1`` (pp_rolling_count): ``cnt`` int32 [m] the number of those windows in which a position
    heads its pair, ``report`` int32 [w1 - w0 + 2] the difference array of the per-window edge counts followed by the status word
    (``flags`` plus ROLLING_LONG_RUN when a pair has ``max_run`` events or more).  Nothing is read back here."""
    dev = require_device(keys, perm, lo, hi, flags)
    m, W = keys.numel(), lo.numel()
    with torch.cuda.device(dev):
        cnt = torch.empty(m, dtype=torch.int32, device=dev)
        report = torch.empty(w1 - w0 + 2, dtype=torch.int32, device=dev)
        check(lib().pp_rolling_count(_p(keys), keys.element_size(), _p(perm), m, _p(lo), _p(hi), W, int(w0), int(w1), int(max_run), _p(flags),
                                     _p(cnt), _p(report), _stream()), "pp_rolling_count")
    return cnt, report


def rolling_fill(keys: torch.Tensor, perm: torch.Tensor, num_nodes: int, lo: torch.Tensor, hi: torch.Tensor, w0: int, w1: int,
                 cnt: torch.Tensor, total: int, out: tuple | None = None):
    """``(edge_index [2, total], edge_weight [total], num_nodes [w1 - w0])`` of the windows ``w0 .. w1 - 1``, window after window and
    (src, dst)-sorted inside one (pp_rolling_fill); ``cnt`` from :func:`rolling_count` over the same windows and ``total`` its sum.
    ``num_nodes`` is an int32 tensor that holds UNSIGNED 32-bit words, as the keys do: a window with node 2^31 - 1 reads 2^31 through
    ``.cpu().numpy().view(numpy.uint32)`` and -2^31 without the view.
    ``out = (index [2, T], weight [T], offset)``: the edges go to columns ``offset .. offset + total - 1`` of these buffers, and the first two
    results are views of them."""
    dev = require_device(keys, perm, lo, hi, cnt)
    m, W, total = keys.numel(), lo.numel(), int(total)
    if total >= _INT32_ROWS:
        raise HipError(f"pp_rolling_fill: {total} edges in one group (2^31 - 16 or more)")
    L = lib()
    with torch.cuda.device(dev):
        if out is None:
            index, weight, offset = torch.empty((2, total), dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.float32, device=dev), 0
        else:
            index, weight, offset = out
            if index.dtype != torch.int64 or weight.dtype != torch.float32 or not index.is_contiguous() or not weight.is_contiguous() \
                    or index.dim() != 2 or index.size(0) != 2 or weight.numel() != index.size(1) or offset < 0 or offset + total > index.size(1):
                raise ValueError("rolling_fill: out must be a contiguous (int64 [2, T], float32 [T], offset) with room for the group")
        nn = torch.empty(w1 - w0, dtype=torch.int32, device=dev)
        ws = _workspace(L.pp_rolling_fill_ws_bytes(m, total), dev)
        src, dst = index[0, offset:], index[1, offset:]
        check(L.pp_rolling_fill(_p(keys), keys.element_size(), _p(perm), m, int(num_nodes), _p(lo), _p(hi), W, int(w0), int(w1), _p(cnt), total,
                                src.data_ptr(), dst.data_ptr(), weight[offset:].data_ptr(), _p(nn), _p(ws), ws.numel(), _stream()),
              "pp_rolling_fill")
    return index[:, offset:offset + total], weight[offset:offset + total], nn


# ------------------------------------------------------------------ random graph models (csrc/pp_random_graphs.hip)
RG_TAG_REGION, RG_TAG_GNM, RG_TAG_WS_DECIDE, RG_TAG_WS_TARGET, RG_TAG_WS_REPAIR = 1, 2, 3, 4, 5      # PP_RG_TAG_* of the header
RG_RECT, RG_STRICT, RG_DIAG, RG_NO_DIAG = 0, 1, 2, 3                                                 # region kinds


def _i64(v: int) -> int:
    """The int64 with the bits of the uint64 ``v`` (seeds, bounds and thresholds cross the C ABI as int64)."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def rg_region_count(regions: torch.Tensor, n_chunks: int, seed: int) -> torch.Tensor:
    """Edges per chunk (int64 ``[n_chunks]``) of the Bernoulli subsets described by ``regions`` (int64 ``[R, 8]``, see the header)."""
    dev = require_device(regions)
    with torch.cuda.device(dev):
        counts = torch.empty(n_chunks, dtype=torch.int64, device=dev)
        check(lib().pp_rg_region_count(_p(regions), regions.size(0), n_chunks, _i64(seed), _p(counts), _stream()), "pp_rg_region_count")
    return counts


def rg_region_fill(regions: torch.Tensor, n_chunks: int, seed: int, offsets: torch.Tensor, total: int, n: int,
                   perm: torch.Tensor | None = None) -> torch.Tensor:
    """The edges themselves, int64 ``[2, total]`` in chunk order; ``offsets`` is the exclusive scan of :func:`rg_region_count`."""
    dev = require_device(regions, offsets, perm)
    with torch.cuda.device(dev):
        out = torch.empty((2, total), dtype=torch.int64, device=dev)
        check(lib().pp_rg_region_fill(_p(regions), regions.size(0), n_chunks, _i64(seed), _p(offsets), _p(perm), n, total, out[0].data_ptr(),
                                      out[1].data_ptr() if total else out.data_ptr(), _stream()), "pp_rg_region_fill")
    return out


def rg_regions_sample(regions: torch.Tensor, n_chunks: int, seed: int, n: int, perm: torch.Tensor | None = None) -> torch.Tensor:
    """count -> scan -> fill with one read-back (the number of edges)."""
    if n_chunks == 0:
        return torch.empty((2, 0), dtype=torch.int64, device=regions.device)
    offsets = exclusive_scan(rg_region_count(regions, n_chunks, seed))
    return rg_region_fill(regions, n_chunks, seed, offsets, int(offsets[-1].item()), n, perm)


def rg_decode(slots: torch.Tensor, kind: int, cols: int) -> torch.Tensor:
    """int64 ``[2, k]``: (row, col) of every slot index of one region shape (``RG_*``; ``cols``: the columns of a rectangle)."""
    slots = slots.contiguous()
    dev = require_device(slots)
    k = slots.numel()
    with torch.cuda.device(dev):
        out = torch.empty((2, k), dtype=torch.int64, device=dev)
        check(lib().pp_rg_decode(_p(slots), k, kind, cols, out[0].data_ptr(), out[1].data_ptr() if k else out.data_ptr(), _stream()), "pp_rg_decode")
    return out


def rg_draws(below: int, seed: int, first: int, count: int, device, tag: int = RG_TAG_GNM, round: int = 0) -> torch.Tensor:
    """The unbiased draws below ``below`` (1 .. 2^64 - 1) with indices ``first .. first + count - 1``; int64 holding the uint64 bits."""
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = torch.empty(count, dtype=torch.int64, device=dev)
        check(lib().pp_rg_draws(_i64(below), _i64(seed), tag, round, first, count, _p(out), _stream()), "pp_rg_draws")
    return out


def rg_first_distinct(values: torch.Tensor, m: int, bits: int):
    """``(distinct, slots)``: the number of distinct values of the draw sequence ``values`` (non-negative, below ``2**bits``) and, if that
    reaches ``m``, the first ``m`` distinct ones in ascending order (else ``None``).  One read-back."""
    dev = require_device(values)
    k = values.numel()
    L = lib()
    sorted_v, draw = sort_pairs(values, None, 0, max(bits, 1))
    with torch.cuda.device(dev):
        first = torch.empty(k, dtype=torch.int32, device=dev)
        check(L.pp_rg_first(_p(sorted_v), _p(draw), k, _p(first), _stream()), "pp_rg_first")
        rank = exclusive_scan(first)
        distinct = int(rank[-1].item())
        if distinct < m:
            return distinct, None
        keep = torch.empty(k, dtype=torch.int32, device=dev)
        check(L.pp_rg_keep(_p(sorted_v), _p(draw), _p(rank), k, m, _p(keep), _stream()), "pp_rg_keep")
        pos = exclusive_scan(keep)
        out = torch.empty(m, dtype=torch.int64, device=dev)
        check(L.pp_rg_compact(_p(sorted_v), _p(pos), k, m, _p(out), _stream()), "pp_rg_compact")
    return distinct, out


def rg_complement(excluded: torch.Tensor, total: int) -> torch.Tensor:
    """The slots of ``[0, total)`` outside the ascending distinct list ``excluded``, ascending."""
    dev = require_device(excluded)
    k = excluded.numel()
    with torch.cuda.device(dev):
        out = torch.empty(total - k, dtype=torch.int64, device=dev)
        check(lib().pp_rg_complement(_p(excluded), k, total - k, _p(out), _stream()), "pp_rg_complement")
    return out


def rg_sorted_keys(edge_index: torch.Tensor, n: int):
    """``(keys, order)``: the keys ``row * n + col`` in ascending order (stable) and, per sorted key, the position of its edge (int32)."""
    ei = edge_index.contiguous()
    dev = require_device(ei)
    k = ei.size(1)
    with torch.cuda.device(dev):
        keys = torch.empty(k, dtype=torch.int64, device=dev)
        check(lib().pp_rg_keys(ei[0].data_ptr(), ei[1].data_ptr() if k else ei.data_ptr(), k, n, _p(keys), _stream()), "pp_rg_keys")
    return sort_pairs(keys, None, 0, max((max(n, 1) * max(n, 1) - 1).bit_length(), 1))


def rg_sort_edges(edge_index: torch.Tensor, n: int) -> torch.Tensor:
    """The edges sorted by (row, col); duplicates stay."""
    _, order = rg_sorted_keys(edge_index, n)
    return edge_index[:, order.to(torch.int64)].contiguous()


def rg_ws_edges(n: int, s: int, seed: int, threshold: int, always: bool, undirected: bool, device) -> torch.Tensor:
    dev = torch.device(device)
    with torch.cuda.device(dev):
        out = torch.empty((2, n * s), dtype=torch.int64, device=dev)
        check(lib().pp_rg_ws_edges(n, s, _i64(seed), _i64(threshold), int(always), int(undirected), out[0].data_ptr(),
                                   out[1].data_ptr() if n * s else out.data_ptr(), _stream()), "pp_rg_ws_edges")
    return out


def rg_ws_repair(edge_index: torch.Tensor, n: int, seed: int, round: int, dups: bool, loops: bool, undirected: bool) -> int:
    """One repair round in place: the surplus copies of an edge (``dups``) and the loops (``loops``) get a new second endpoint drawn for
    (edge position, ``round``).  Returns the number of offenders it found (0: nothing was changed)."""
    dev = require_device(edge_index)
    k = edge_index.size(1)
    sorted_k, order = rg_sorted_keys(edge_index, n)
    L = lib()
    with torch.cuda.device(dev):
        flag = torch.empty(k, dtype=torch.int32, device=dev)
        check(L.pp_rg_ws_offenders(_p(sorted_k), _p(order), k, n, int(dups), int(loops), _p(flag), _stream()), "pp_rg_ws_offenders")
        offenders = int(exclusive_scan(flag)[-1].item())
        if offenders:
            check(L.pp_rg_ws_redraw(n, k, _i64(seed), round, int(undirected), _p(flag), edge_index[0].data_ptr(), edge_index[1].data_ptr(), _stream()),
                  "pp_rg_ws_redraw")
    return offenders


# degree-sequence models: the header's "Degree-sequence models" block, DESIGN.md for the rules
RG_TAG_MR_SHUFFLE, RG_TAG_MR_VICTIM, RG_TAG_MR_SIDE = 6, 7, 8


def rg_eg_check(degrees: torch.Tensor) -> bool:
    """Whether the int64 degrees, ALL IN ``0 .. n - 1``, meet the Erdös-Gallai condition for r = 1 .. n and have an even sum (one read-back)."""
    dev = require_device(degrees)
    n = degrees.numel()
    asc = sort_pairs(degrees, None, 0, max((n - 1).bit_length(), 1))[0] if n > 1 else degrees.contiguous()
    scan = exclusive_scan(asc)
    with torch.cuda.device(dev):
        violated = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib().pp_rg_eg_check(_p(asc), _p(scan), n, _p(violated), _stream()), "pp_rg_eg_check")
        return int(violated.item()) == 0


def rg_mr_matching(ptr: torch.Tensor, n: int, stubs: int, seed: int) -> torch.Tensor:
    """The first matching, int64 ``[2, stubs / 2]`` with sorted ends: the stubs of ``ptr`` (the exclusive scan of n degrees, ``ptr[n] == stubs``,
    even) in the stable order of their 64-bit shuffle keys, neighbours joined."""
    dev = require_device(ptr)
    with torch.cuda.device(dev):
        node = torch.empty(stubs, dtype=torch.int32, device=dev)
        key = torch.empty(stubs, dtype=torch.int64, device=dev)
        check(lib().pp_rg_mr_stubs(_p(ptr), n, stubs, _i64(seed), _p(node), _p(key), _stream()), "pp_rg_mr_stubs")
        _, order = sort_pairs(key, None, 0, 64)
        out = torch.empty((2, stubs // 2), dtype=torch.int64, device=dev)
        check(lib().pp_rg_mr_pair(_p(node), _p(order), stubs // 2, n, out[0].data_ptr(), out[1].data_ptr() if stubs // 2 else out.data_ptr(), _stream()),
              "pp_rg_mr_pair")
    return out


def rg_mr_repair(edge_index: torch.Tensor, n: int, seed: int, round: int, multi: bool) -> int:
    """One repair round in place: loops and (unless ``multi``) surplus copies claim a victim edge each and exchange ends with it where that
    makes nothing worse.  Returns the number of offenders it found (0: nothing was changed).  One read-back."""
    dev = require_device(edge_index)
    k = edge_index.size(1)
    sorted_k, order = rg_sorted_keys(edge_index, n)
    L = lib()
    with torch.cuda.device(dev):
        flag = torch.empty(k, dtype=torch.int32, device=dev)
        check(L.pp_rg_ws_offenders(_p(sorted_k), _p(order), k, n, int(not multi), 1, _p(flag), _stream()), "pp_rg_ws_offenders")
        offenders = int(exclusive_scan(flag)[-1].item())
        if offenders:
            claim = torch.empty(k, dtype=torch.int32, device=dev)                  # (uint32 on the device)
            check(L.pp_rg_mr_claim(_p(flag), k, _i64(seed), round, _p(claim), _stream()), "pp_rg_mr_claim")
            check(L.pp_rg_mr_swap(_p(flag), _p(claim), _p(sorted_k), k, n, _i64(seed), round, int(multi), edge_index[0].data_ptr(),
                                  edge_index[1].data_ptr(), _stream()), "pp_rg_mr_swap")
    return offenders


# ------------------------------------------------------------------ random walks (csrc/pp_walks.hip)
RG_TAG_WALK_START, RG_TAG_WALK_STEP = 10, 11                       # PP_RG_TAG_WALK_* of the header
WALK_START_GIVEN, WALK_START_WEIGHTED, WALK_START_UNIFORM = 0, 1, 2


def walk_check_sizes(n: int, m: int, walks: int, steps: int, order: int) -> None:
    """The size limits of the walk kernels (host arithmetic, nothing is allocated): raises like the kernels would."""
    check(lib().pp_walk_check_sizes(n, m, walks, steps, order), "pp_walk_check_sizes")


class WalkTable(NamedTuple):
    cum: torch.Tensor            # [m] float64: row-local running sums of the weights
    total: torch.Tensor          # [n] float64: T_v
    bad: bool                    # a weight was negative or not finite (or a row's sum overflowed)


def walk_table(row_ptr: torch.Tensor, n: int, m: int, weight: torch.Tensor | None) -> WalkTable:
    """The transition table of ``pp_walk_table``; one read-back (the flag)."""
    dev = require_device(row_ptr, weight)
    if weight is not None and weight.dtype not in (torch.float32, torch.float64):
        raise TypeError("walk_table: float32 or float64 weights")
    with torch.cuda.device(dev):
        cum = torch.empty(m, dtype=torch.float64, device=dev)
        total = torch.empty(n, dtype=torch.float64, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        code = _DTYPE_CODE[weight.dtype] if weight is not None else _DTYPE_CODE[torch.float64]
        check(lib().pp_walk_table(_p(row_ptr), n, m, _p(weight), code, _p(cum), _p(total), _p(bad), _stream()), "pp_walk_table")
        return WalkTable(cum, total, bool(bad.item()))


def walk_start_table(total: torch.Tensor):
    """``(bcum [n], B [blocks])`` of ``pp_walk_start_table``: running sums of T_v inside blocks of 1024 nodes, and of the blocks' totals."""
    dev = require_device(total)
    n = total.numel()
    with torch.cuda.device(dev):
        bcum = torch.empty(n, dtype=torch.float64, device=dev)
        B = torch.empty(int(lib().pp_walk_start_blocks(n)), dtype=torch.float64, device=dev)
        check(lib().pp_walk_start_table(_p(total), n, _p(bcum), _p(B), _stream()), "pp_walk_start_table")
    return bcum, B


def walk_positive_nodes(total: torch.Tensor) -> torch.Tensor:
    """The nodes with T_v > 0, ascending (int32): flag -> scan -> compact, one read-back (their number)."""
    dev = require_device(total)
    n = total.numel()
    with torch.cuda.device(dev):
        flag = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib().pp_walk_positive_flag(_p(total), n, _p(flag), _stream()), "pp_walk_positive_flag")
        pos = exclusive_scan(flag)
        count = int(pos[-1].item())
        out = torch.empty(count, dtype=torch.int32, device=dev)
        check(lib().pp_walk_positive_list(_p(pos), n, count, _p(out), _stream()), "pp_walk_positive_list")
    return out


def walk_run(row_ptr: torch.Tensor, col: torch.Tensor, table: WalkTable, n: int, walks: int, steps: int, order: int, seed: int, mode: int,
             start_nodes: torch.Tensor | None = None, start_table=None, positive: torch.Tensor | None = None):
    """``(nodes [steps + 1, walks] int32 step-major, lengths [walks] int32)`` of ``pp_walk_run``."""
    dev = require_device(row_ptr, col, table.cum, table.total, start_nodes, positive)
    m = col.numel()
    walk_check_sizes(n, m, walks, steps, order)
    bcum, B = start_table if start_table is not None else (None, None)
    with torch.cuda.device(dev):
        nodes = torch.empty((steps + 1, walks), dtype=torch.int32, device=dev)
        lengths = torch.empty(walks, dtype=torch.int32, device=dev)
        check(lib().pp_walk_run(_p(row_ptr), _p(col), _p(table.cum), _p(table.total), n, m, walks, steps, order, _i64(seed), mode, _p(start_nodes),
                                _p(bcum), _p(B), _p(positive), 0 if positive is None else positive.numel(), _p(nodes), _p(lengths), _stream()),
              "pp_walk_run")
    return nodes, lengths


class WalkStore(NamedTuple):
    node_sequence: torch.Tensor  # [P, 1] int64
    edge_index: torch.Tensor     # [2, P - kept] int64
    dag_num_nodes: torch.Tensor  # [kept] int64
    dag_num_edges: torch.Tensor  # [kept] int64
    dag_weight: torch.Tensor     # [kept] float32


def walk_pack(nodes: torch.Tensor, lengths: torch.Tensor, node_sequence: torch.Tensor, n: int) -> WalkStore:
    """The ``PathData`` tensors of a batch (``pp_walk_pack_count`` -> two scans -> ``pp_walk_pack_fill``); one read-back (the two totals)."""
    dev = require_device(nodes, lengths, node_sequence)
    steps, walks = nodes.size(0) - 1, nodes.size(1)
    order = node_sequence.size(1)
    L = lib()
    with torch.cuda.device(dev):
        keep = torch.empty(walks, dtype=torch.int32, device=dev)
        count = torch.empty(walks, dtype=torch.int32, device=dev)
        check(L.pp_walk_pack_count(_p(lengths), walks, steps, order, _p(keep), _p(count), _stream()), "pp_walk_pack_count")
        offset, rank = exclusive_scan(count), exclusive_scan(keep)
        positions, kept = torch.stack((offset[-1], rank[-1])).tolist()
        seq = torch.empty((positions, 1), dtype=torch.int64, device=dev)
        edges = torch.empty((2, positions - kept), dtype=torch.int64, device=dev)
        dag_nodes = torch.empty(kept, dtype=torch.int64, device=dev)
        dag_edges = torch.empty(kept, dtype=torch.int64, device=dev)
        dag_weight = torch.empty(kept, dtype=torch.float32, device=dev)
        check(L.pp_walk_pack_fill(_p(nodes), _p(lengths), walks, steps, order, n, _p(node_sequence), _p(offset), _p(rank), positions, kept, _p(seq),
                                  edges[0].data_ptr(), edges[1].data_ptr() if kept else edges.data_ptr(), _p(dag_nodes), _p(dag_edges),
                                  _p(dag_weight), _stream()), "pp_walk_pack_fill")
    return WalkStore(seq, edges, dag_nodes, dag_edges, dag_weight)


# ------------------------------------------------------------------ distributions and PageRank (csrc/pp_graph_diffusion.hip)
DIFFUSION_PAGERANK, DIFFUSION_WALK = 0, 1                          # PP_DIFFUSION_* of the header
DIFFUSION_MAX_WIDTH = 64                                           # columns per launch; a wider batch runs in tiles


def diffusion_heavy_min() -> int:
    """The pull-list length from which the propagator gives a row a whole workgroup (the library's default)."""
    return int(lib().pp_diffusion_heavy_min())


def diffusion_width(columns: int) -> int:
    """The padded width of a block of ``columns`` (1 .. 64) distributions: the next power of two."""
    if not 1 <= columns <= DIFFUSION_MAX_WIDTH:
        raise ValueError(f"a block holds 1 .. {DIFFUSION_MAX_WIDTH} columns, got {columns}")
    return 1 << (columns - 1).bit_length()


def diffusion_check_sizes(n: int, k: int, width: int, kept: int, device=None) -> None:
    """The size limits of the propagator (host arithmetic, nothing is allocated): raises like the kernels would; with ``device`` also when
    the ``kept`` blocks are more than that device's memory."""
    check(lib().pp_diffusion_check_sizes(n, k, width, kept), "pp_diffusion_check_sizes")
    if device is not None:
        need, have = n * width * 8 * kept, torch.cuda.get_device_properties(device).total_memory
        if need > have:
            raise HipError(f"pp_diffusion_check_sizes failed with status -4: {kept} blocks of {n} x {width} float64 are {need} bytes, the "
                           f"device has {have}")


class DiffusionTable(NamedTuple):
    total: torch.Tensor          # [n] float64: T_u
    prob: torch.Tensor           # [k] float64, pull order: w / T_u
    dangling: torch.Tensor       # [n] uint8: !(T_u > 0)
    bad: bool                    # a weight was negative or not finite (or a row's sum overflowed)


def diffusion_table(row_ptr: torch.Tensor, weight: torch.Tensor | None, src: torch.Tensor, perm: torch.Tensor, n: int) -> DiffusionTable:
    """The transition table of ``pp_diffusion_table``; one read-back (the flag)."""
    dev = require_device(row_ptr, weight, src, perm)
    k = src.numel()
    if weight is not None and (weight.dtype != torch.float64 or weight.numel() != k):
        raise ValueError(f"weight must be a float64 vector of {k} entries")
    if row_ptr.numel() != n + 1 or perm.numel() != k:
        raise ValueError("row_ptr must have n + 1 entries and perm one per pull entry")
    row_ptr, src, perm = (t.to(torch.int64).contiguous() for t in (row_ptr, src, perm))
    weight = None if weight is None else weight.contiguous()
    with torch.cuda.device(dev):
        total = torch.empty(n, dtype=torch.float64, device=dev)
        prob = torch.empty(k, dtype=torch.float64, device=dev)
        dangling = torch.empty(n, dtype=torch.uint8, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib().pp_diffusion_table(_p(row_ptr), _p(weight), _p(src), _p(perm), n, k, _p(total), _p(prob), _p(dangling), _p(bad), _stream()),
              "pp_diffusion_table")
        return DiffusionTable(total, prob, dangling, bool(bad.item()))


class DiffusionRun(NamedTuple):
    final: torch.Tensor          # [n, B] float64: per column the iterate that met the criterion, or the last one
    iterations: list             # [B] iterations done per column
    converged: list              # [B] the criterion held
    trajectory: torch.Tensor | None     # [max_iter + 1, n, B] with keep_all
    tvd: torch.Tensor | None     # [max_iter + 1, B] with a target
    grids: tuple                 # workgroups of the row launch and of the heavy launch


def diffusion_run(col_ptr: torch.Tensor, src: torch.Tensor, table: DiffusionTable, n: int, mode: int, start: torch.Tensor, threshold: float,
                  max_iter: int, alpha: float = 0.0, lazy: float = 0.0, p: torch.Tensor | None = None, d: torch.Tensor | None = None,
                  target: torch.Tensor | None = None, keep_all: bool = False, want_tvd: bool = False, batch: int = 0,
                  heavy_min: int = 0) -> DiffusionRun:
    """``pp_diffusion_run`` on one block of at most 64 columns: ``start``, ``p``, ``d`` float64 ``[n, B]``, ``target`` float64 ``[n]``.  A
    negative ``threshold`` runs exactly ``max_iter`` iterations.  The block is padded to a power of two with zero columns."""
    if start.dim() != 2 or start.size(0) != n or start.dtype != torch.float64:
        raise ValueError(f"start must be float64 [n = {n}, B], got {tuple(start.shape)} {start.dtype}")
    B = int(start.size(1))
    width = diffusion_width(B)
    k = src.numel()
    max_iter = int(max_iter)
    kept = max_iter + 1 if keep_all else 2
    for t, name in ((p, "p"), (d, "d")):
        if t is not None and (t.shape != start.shape or t.dtype != torch.float64):
            raise ValueError(f"{name} must be float64 {tuple(start.shape)}")
    if target is not None and (target.dtype != torch.float64 or target.numel() != n):
        raise ValueError(f"target must be a float64 vector of {n} entries")
    if mode == DIFFUSION_PAGERANK and (p is None or d is None):
        raise ValueError("PageRank needs p and d")
    if want_tvd and target is None:
        raise ValueError("tvd needs a target")
    dev = require_device(col_ptr, src, table.prob, table.dangling, start, p, d, target)
    diffusion_check_sizes(n, k, width, kept, dev)
    L = lib()
    with torch.cuda.device(dev):
        def padded(t):
            if t is None:
                return None
            if width == B:
                return t.contiguous()
            out = torch.zeros((n, width), dtype=torch.float64, device=dev)
            out[:, :B] = t
            return out
        X = torch.empty((kept, n, width), dtype=torch.float64, device=dev)
        if width != B:
            X[0].zero_()
        X[0, :, :B] = start
        p_pad = padded(p)
        d_pad = p_pad if d is p else padded(d)
        target = None if target is None else target.reshape(-1).contiguous()
        tvd = torch.zeros((max_iter + 1, width), dtype=torch.float64, device=dev) if want_tvd else None
        iterations, converged = (ctypes.c_int64 * width)(), (ctypes.c_int64 * width)()
        where, grids = ctypes.c_int64(0), (ctypes.c_int64 * 2)()
        ws = _workspace(L.pp_diffusion_ws_bytes(n, width), dev)
        check(L.pp_diffusion_run(_p(col_ptr), _p(src), _p(table.prob), _p(table.dangling), n, k, width, B, int(mode), float(alpha), float(lazy),
                                 _p(p_pad), _p(d_pad), _p(target), _p(X), kept, float(threshold), max_iter, int(batch), int(heavy_min),
                                 ctypes.addressof(iterations), ctypes.addressof(converged), ctypes.addressof(where), _p(tvd),
                                 ctypes.addressof(grids), _p(ws), ws.numel(), _stream()), "pp_diffusion_run")
        final = X[int(where.value), :, :B]
        return DiffusionRun(final.contiguous() if width != B or not keep_all else final, list(iterations[:B]), [bool(c) for c in converged[:B]],
                            X[:, :, :B] if keep_all else None, None if tvd is None else tvd[:, :B], (int(grids[0]), int(grids[1])))


def diffusion_project(ptr: torch.Tensor, idx: torch.Tensor, rows: int, x: torch.Tensor, heavy_min: int = 0) -> torch.Tensor:
    """``pp_diffusion_project``: float64 ``[rows, B]`` = the sums of the rows ``idx[ptr[r] : ptr[r + 1]]`` of ``x`` (float64 ``[n_src, B]``,
    B <= 64)."""
    if x.dim() != 2 or x.dtype != torch.float64:
        raise ValueError("x must be float64 [n, B]")
    n_src, B = int(x.size(0)), int(x.size(1))
    width = diffusion_width(B)
    dev = require_device(ptr, idx, x)
    ptr, idx = ptr.to(torch.int64).contiguous(), idx.to(torch.int64).contiguous()
    if ptr.numel() != rows + 1:
        raise ValueError(f"ptr must have rows + 1 = {rows + 1} entries")
    k = idx.numel()
    L = lib()
    with torch.cuda.device(dev):
        if width != B:
            xp = torch.zeros((n_src, width), dtype=torch.float64, device=dev)
            xp[:, :B] = x
        else:
            xp = x.contiguous()
        out = torch.empty((rows, width), dtype=torch.float64, device=dev)
        ws = _workspace(L.pp_diffusion_ws_bytes(rows, width), dev)
        check(L.pp_diffusion_project(_p(ptr), _p(idx), rows, n_src, k, _p(xp), width, _p(out), int(heavy_min), _p(ws), ws.numel(), _stream()),
              "pp_diffusion_project")
    return out if width == B else out[:, :B].contiguous()
