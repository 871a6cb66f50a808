"""numpy stand-in of the two device contracts ``core/multi_order_passes.continue_in_passes`` adds to those of the N-rank build
(``tests/cpu_ops_multiorder.py``): the split of a level into parts of whole types and the concatenation of the parts' layer pieces.

Same arguments, same results as ``pathpyg_amd._hip.multi_order_split / multi_order_concat``.  ``ibase`` may be an int32 array that has
WRAPPED (what the device scan leaves for a level of 2^31 or more children) or the stand-in's own int64 prefix: the per-type counts are the
differences modulo 2^32 either way, every single count being below 2^31."""
from __future__ import annotations

import numpy as np
import torch

from pathpyg_amd._hip import _INT32_ROWS, SPLIT_MAX_PARTS, MultiOrderLevel
from pathpyg_amd.core.multi_order_passes import greedy_cuts
from tests.cpu_ops_multiorder import CpuOpsMultiOrder


def counts_from_ibase(ibase: np.ndarray) -> np.ndarray:
    """True per-type child counts (int64) from a prefix stored in int32 (possibly wrapped) or int64."""
    return np.diff(np.asarray(ibase).astype(np.int64)) & 0xffffffff


class CpuOpsPasses(CpuOpsMultiOrder):
    name = "cpu-multiorder-passes"

    @staticmethod
    def multi_order_split(level, budget):
        counts = counts_from_ibase(level.ibase)
        assert (counts < 1 << 31).all()
        prefix = np.concatenate(([0], np.cumsum(counts)))
        assert int(prefix[-1]) == int(level.children), "the level's true children against its own prefix"
        if min(int(level.types), 2 * (int(level.children) // int(budget)) + 2) > SPLIT_MAX_PARTS:
            raise ValueError("multi_order_split: more parts than one split makes")
        cuts = greedy_cuts(prefix.tolist(), int(budget))
        tptr = np.asarray(level.tptr).astype(np.int64)
        parts = []
        for t0, t1 in zip(cuts, cuts[1:]):
            if int(prefix[t1] - prefix[t0]) >= _INT32_ROWS:
                return None
            i0, i1 = int(tptr[t0]), int(tptr[t1])
            inst = tuple(a[i0:i1] for a in level.inst)          # (views)
            parts.append(MultiOrderLevel(types=t1 - t0, children=int(prefix[t1] - prefix[t0]), status=0, tptr=tptr[t0: t1 + 1] - tptr[t0],
                                         ibase=prefix[t0: t1 + 1] - prefix[t0], inst=inst, row_ptr=None, col=level.col[t0:t1],
                                         weight=None if level.weight is None else level.weight[t0:t1],
                                         tlast=None if level.tlast is None else level.tlast[t0:t1]))
        return parts

    @staticmethod
    def multi_order_concat(pieces, want_last):
        rows, cols, weights, lasts = [], [], [], []
        edges = 0
        for n_rows, b in pieces:
            if b is None:
                rows.append(torch.full((n_rows,), edges, dtype=torch.int64))
                continue
            assert b.row_ptr.numel() == n_rows + 1 and int(b.row_ptr[-1]) == b.types
            rows.append(b.row_ptr[:n_rows].long() + edges)
            cols.append(b.col[:b.types])
            weights.append(b.weight[:b.types])
            if want_last:
                lasts.append(b.tlast[:b.types])
            edges += b.types
        assert edges < _INT32_ROWS
        row_ptr = torch.cat(rows + [torch.tensor([edges])]).to(torch.int32)
        return row_ptr, torch.cat(cols), torch.cat(weights), torch.cat(lasts) if want_last else None
