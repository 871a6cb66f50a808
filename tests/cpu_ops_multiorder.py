"""torch / numpy stand-in of the four device contracts of ``distributed.build_multi_order_shard`` (node loads, level 1 on a node range, one
step, the stitch), so that the protocol — cuts, rebasing, empty ranks, agreement on fallbacks — runs without a GPU and under ``gloo``.

Same arguments, same results as ``pathpyg_amd._hip.multi_order_node_loads / _prepare_range / _step / _stitch``, the status bits and the
4096-children limit of ``pp_multiorder_step`` included.  The level arrays the driver never looks into (``tptr``, ``ibase``, ``inst``, ``tab``)
are numpy arrays here.  Merged weights are summed in float64 and rounded once: equal to the kernels' left-to-right float32 sum whenever
every partial sum is exact in float32 (unit and dyadic weights, which is what the tests feed it).  Integer timestamps only."""
from __future__ import annotations

import numpy as np
import torch

from pathpyg_amd._hip import MultiOrderLevel
from tests.cpu_ops import CpuOpsNode

BIG = 4096                 # kMoBigMax of csrc/pp_multiorder.hip: children of one type a workgroup sorts
OVERFLOW, BAD_INDEX = 4, 1
I32_MAX = 0x7fffffff


def _run_sums(values: np.ndarray, starts: np.ndarray) -> np.ndarray:
    return np.add.reduceat(values, starts) if values.size else values[:0]


class CpuOpsMultiOrder(CpuOpsNode):
    name = "cpu-multiorder"

    @staticmethod
    def gather_concat(rows, idx, suffix):
        return torch.cat((rows[idx], suffix.unsqueeze(1)), dim=1)

    @staticmethod
    def multi_order_node_loads(edge_index, time, num_nodes, delta, weight=None):
        ei = edge_index.numpy().astype(np.int64)
        t = time.numpy()
        m, n = ei.shape[1], int(num_nodes)
        if m == 0 or n == 0 or t.dtype.kind != "i" or (weight is not None and weight.dtype != torch.float32):
            return None
        if np.any(t[1:] < t[:-1]):
            return None
        status = BAD_INDEX if (ei.min() < 0 or ei.max() >= n) else 0
        src, dst = np.clip(ei[0], 0, n - 1), np.clip(ei[1], 0, n - 1)
        ids = np.argsort(src, kind="stable")                       # events grouped by source, time order inside
        rowptr = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n))))
        # window of event e: the events of its head node's list with t_e < t <= t_e + delta (one sorted key per list position)
        t0 = int(t.min())
        span = int(t.max()) - t0 + int(delta) + 2
        list_key = src[ids] * span + (t[ids] - t0)
        first = np.searchsorted(list_key, dst * span + (t - t0), side="right")
        end = np.searchsorted(list_key, dst * span + (t - t0) + int(delta), side="right")
        count = (end - first).astype(np.int64)
        loads = np.zeros((2, n + 1), dtype=np.int64)
        loads[0] = rowptr
        loads[1] = np.concatenate(([0], np.cumsum(count[ids])))[rowptr]
        w = np.ones(m, dtype=np.float32) if weight is None else weight.numpy().astype(np.float32)
        tab = np.stack((dst[ids], first[ids], count[ids], ids), axis=1)
        windows = dict(src=src, dst=dst, ids=ids, first=first, count=count, w=w, weighted=weight is not None, n=n, status=status, tab=tab)
        return windows, torch.from_numpy(loads)

    @staticmethod
    def multi_order_prepare_range(windows, node_lo, node_hi, p_lo, m_own):
        wd = windows
        own = wd["ids"][p_lo: p_lo + m_own]
        src, dst = wd["src"][own], wd["dst"][own]
        assert src.min() >= node_lo and src.max() < node_hi
        order = np.lexsort((dst, src))                             # stable: time order inside a node pair
        ev, src, dst = own[order], src[order], dst[order]
        head = np.ones(m_own, dtype=bool)
        head[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
        starts = np.flatnonzero(head)
        types = starts.size
        cc = wd["count"][ev]
        csum = _run_sums(cc, starts)
        status = wd["status"] | (OVERFLOW if (csum > I32_MAX).any() else 0)
        weight = _run_sums(wd["w"][ev].astype(np.float64), starts) if wd["weighted"] else np.diff(np.append(starts, m_own)).astype(np.float64)
        n_own = node_hi - node_lo
        row_ptr = np.concatenate(([0], np.cumsum(np.bincount(src[starts] - node_lo, minlength=n_own))))
        tlast = torch.from_numpy(dst[starts].astype(np.int32))
        level = MultiOrderLevel(types=int(types), children=int(csum.sum()), status=int(status), tptr=np.append(starts, m_own),
                                ibase=np.concatenate(([0], np.cumsum(csum))), inst=(wd["first"][ev], cc, wd["w"][ev]),
                                row_ptr=torch.from_numpy(row_ptr.astype(np.int32)), col=tlast, weight=torch.from_numpy(weight.astype(np.float32)),
                                tlast=tlast)
        return level, wd["tab"]

    @staticmethod
    def multi_order_step(level, cand_ptr, cand_last, tab, weighted, last, clock=None, name="layer"):
        T, total = level.types, level.children
        assert T > 0 and total > 0
        cf, cc, w = level.inst
        n_inst = cf.size
        type_of_inst = np.repeat(np.arange(T), np.diff(level.tptr))
        parent = np.repeat(np.arange(n_inst), cc)
        first_child = np.concatenate(([0], np.cumsum(cc)))[:-1]
        src = cf[parent] + (np.arange(total) - first_child[parent])
        s, d = type_of_inst[parent], tab[src, 0]
        status = OVERFLOW if (np.diff(level.ibase) > BIG).any() else 0
        order = np.lexsort((d, s))                                 # stable sort by the new last node inside every parent type
        s, d, src, w_child = s[order], d[order], src[order], w[parent][order]
        head = np.ones(total, dtype=bool)
        head[1:] = (s[1:] != s[:-1]) | (d[1:] != d[:-1])
        starts = np.flatnonzero(head)
        new_types = starts.size
        row_ptr = np.concatenate(([0], np.cumsum(np.bincount(s[starts], minlength=T))))
        # column of (s -> s ++ d): the edge (suffix(s), d) of the finished layer — looked up in the GLOBAL tables
        cp, cl = cand_ptr.numpy().astype(np.int64), cand_last.numpy().astype(np.int64)
        big = int(max(cl.max(initial=0), d.max(initial=0))) + 1
        cand_key = np.repeat(np.arange(cp.size - 1), np.diff(cp)) * big + cl
        want = level.col.numpy().astype(np.int64)[s[starts]] * big + d[starts]
        col = np.searchsorted(cand_key, want)
        assert (col < cand_key.size).all() and (cand_key[col] == want).all(), "the suffix of a path is a path"
        weight = _run_sums(w_child.astype(np.float64), starts) if weighted else np.diff(np.append(starts, total)).astype(np.float64)
        ccc = tab[src, 2]
        csum = _run_sums(ccc, starts)
        if (csum > I32_MAX).any():
            status |= OVERFLOW
        tlast = torch.from_numpy(d[starts].astype(np.int32))
        return MultiOrderLevel(types=int(new_types), children=0 if last else int(csum.sum()), status=int(status),
                               tptr=None if last else np.append(starts, total), ibase=None if last else np.concatenate(([0], np.cumsum(csum))),
                               inst=None if last else (tab[src, 1], ccc, w_child), row_ptr=torch.from_numpy(row_ptr.astype(np.int32)),
                               col=torch.from_numpy(col.astype(np.int32)), weight=torch.from_numpy(weight.astype(np.float32)),
                               tlast=None if last else tlast)

    @staticmethod
    def multi_order_stitch(gathered, stride, last_at, row_lo, edge_lo):
        world = len(row_lo) - 1
        blocks = gathered[: world * stride].view(world, stride)
        rows = [blocks[r, : row_lo[r + 1] - row_lo[r]] + edge_lo[r] for r in range(world)]
        cand_ptr = torch.cat(rows + [torch.tensor([edge_lo[-1]], dtype=torch.int32)]).to(torch.int32)
        cand_last = torch.cat([blocks[r, last_at: last_at + edge_lo[r + 1] - edge_lo[r]] for r in range(world)])
        return cand_ptr, cand_last
