"""De Bruijn layers whose levels do not fit one step, built in PASSES over contiguous ranges of types (one GPU).

The level-by-level builder (csrc/pp_multiorder.hip) keeps a level's instances grouped by type and numbers them with int32: one step takes
fewer than 2^31 - 16 child instances.  Nothing in the algorithm needs more: the children of a type depend on that type's instances only,
instance records point into the global continuation table, columns are positions in the finished layer's global tables.  Any contiguous
range of a level's types, renumbered from 0, is a valid input of the unchanged step — what a rank of the split by first node is given
(``distributed.build_multi_order_shard``).  Here one device takes the ranges one after another:

* **split**: every part of the level with more children than the budget is cut into parts of whole types (``ops.multi_order_split``:
  greedy, deterministic; the per-type counts are taken in 64 bits from the possibly wrapped int32 ``ibase``); the parts are views;
* **step**: the unchanged ``ops.multi_order_step`` per part that has children, with the global candidate tables; a part without children
  contributes empty rows;
* **concat**: the parts' pieces, in part order, into the layer's global ``row_ptr`` / ``col`` / ``weight`` / ``last``
  (``ops.multi_order_concat``) — the finished layer AND the next level's candidate tables.  Finished layers are never split, only level state.

Only three things stay bounded by int32: a part's instances, a layer's edges, one type's children (4096).  Written against an ``ops``
object (``pathpyg_amd._hip`` itself on the device, a numpy stand-in in the tests), as the N-rank build is.
"""
from __future__ import annotations

from .. import _hip


def greedy_cuts(prefix, budget: int) -> list[int]:
    """The cut rule on the host, for a prefix ``[T + 1]`` of per-type child counts (any sequence of ints): a part that starts at type ``t0``
    ends before the first type ``t`` with ``prefix[t + 1] - prefix[t0] > budget`` and holds at least one type.  Returns the first type of
    every part and ``T``.  (What ``pp_multiorder_split`` computes on the device; the stand-in of the tests calls this.)"""
    n = len(prefix) - 1
    cuts = [0]
    while cuts[-1] < n:
        t0 = cuts[-1]
        t = t0
        while t < n and int(prefix[t + 1]) - int(prefix[t0]) <= budget:
            t += 1
        cuts.append(max(t, t0 + 1))
    return cuts


def continue_in_passes(ops, level, cand_ptr, cand_last, tab, layers: list, max_order: int, weighted: bool, budget: int, clock=None):
    """The layers ``len(layers) + 1 .. max_order`` from ``level`` = level ``len(layers)`` (its layer is ``layers[-1]``, ``cand_ptr`` /
    ``cand_last`` that layer's row pointers and last nodes, ``tab`` the stream's continuation table), in passes of at most ``budget`` child
    instances (a single type with more is a pass of its own).  Returns ``(layers, passes, cuts)`` — ``layers`` extended by one
    :class:`~pathpyg_amd._hip.MultiOrderLayer` per order with true Python-int ``n_instances``, ``passes[j]`` the number of parts of the
    j-th level taken here, ``cuts[j]`` their first types (global type ids of that level) and the level's type count — or ``None`` where the
    generic kernels have to take over: a type with more than 4096 children (status bit 2 of a part), a layer without edges, a layer with
    2^31 - 16 or more edges.  Read-backs: one per part and step, one per split."""
    limit = _hip._INT32_ROWS                            # what one step numbers, and what a layer's int32 edge ids hold
    budget = max(1, min(int(budget), limit - 1))
    layers = list(layers)
    parts = [level]
    passes, cuts = [], []

    def timed(name, fn, *args):
        # (``clock`` as in _hip.multi_order_temporal: device events around the split and the concat of a level; the steps record their own)
        if clock is None:
            return fn(*args)
        import torch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn(*args)
        t1.record()
        clock.append((name, t0, t1))
        return out

    for k in range(len(layers) + 1, max_order + 1):
        top = k == max_order
        split = []
        for part in parts:
            if part.children > budget and part.types > 1:
                pieces = timed(f"split {k}", ops.multi_order_split, part, budget)
                if pieces is None:
                    return None
                split.extend(pieces)
            elif part.children >= limit:
                return None
            else:
                split.append(part)
        bounds = [0]
        for part in split:
            bounds.append(bounds[-1] + part.types)
        pieces = []
        for part in split:
            if part.types > 0 and part.children > 0:
                nxt = ops.multi_order_step(part, cand_ptr, cand_last, tab, weighted, top, clock, f"layer {k}")
                if nxt.status & 4:
                    return None
                if not top and hasattr(nxt.tptr, "clone") and nxt.tptr.numel() > 2 * (nxt.types + 1):
                    # the step sized them for as many types as children: 8 B per instance that would stay for the whole next level
                    nxt.tptr, nxt.ibase = nxt.tptr[:nxt.types + 1].clone(), nxt.ibase[:nxt.types + 1].clone()
            else:
                nxt = None
            pieces.append((part.types, nxt))
        n_edges = sum(nxt.types for _, nxt in pieces if nxt is not None)
        if n_edges == 0 or n_edges >= limit:
            return None
        row_ptr, col, weight, last = timed(f"concat {k}", ops.multi_order_concat, pieces, not top)
        layers.append(_hip.MultiOrderLayer(n_nodes=bounds[-1], n_edges=n_edges, n_instances=sum(part.children for part in split), row_ptr=row_ptr,
                                           col=col, weight=weight, last=last))
        passes.append(len(split))
        cuts.append(bounds)
        if top:
            break
        # the next level's parts keep their own instances; what they share with the finished layer becomes a view of it
        parts, at = [], 0
        for _, nxt in pieces:
            if nxt is None or nxt.types == 0:
                continue
            nxt.col, nxt.weight, nxt.tlast, nxt.row_ptr = col[at: at + nxt.types], weight[at: at + nxt.types], last[at: at + nxt.types], None
            at += nxt.types
            parts.append(nxt)
        cand_ptr, cand_last = row_ptr, last
    return layers, passes, cuts
