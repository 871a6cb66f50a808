"""TEST-ONLY stand-ins for the operations that the semi-supervised loop adds to :class:`pathpyg_amd.nn.sharded.HipOps` — one rank's masked
cross-entropy sums, their finish, its confusion counters, and the first GCN layer on implicit one-hot features — on torch-CPU, so that the
collectives of ``ShardedDBGNN.loss(mask=...)`` / ``evaluate`` and the row-map bookkeeping run under ``gloo`` and ``ThreadWorld`` without a GPU.
Written from the kernels' CONTRACTS (include/pathpyg_amd.h), not from their code.  Nothing under ``pathpyg_amd/`` imports this file."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.cpu_ops import CpuOps, CpuOpsNode


class _SemiOps:
    @staticmethod
    def _selected(target, mask, ignore_index):
        keep = torch.ones(target.size(0), dtype=torch.bool) if mask is None else mask.clone()
        if ignore_index is not None:
            keep &= target != ignore_index
        return keep

    @staticmethod
    def masked_sums(logits, target, mask, weight, ignore_index, want_grad):
        c = logits.size(1)
        keep = _SemiOps._selected(target, mask, ignore_index)
        bad = keep & ((target < 0) | (target >= c))
        valid = keep & ~bad
        y = target.clamp(0, c - 1)
        w = (torch.ones(c) if weight is None else weight.float())[y] * valid
        z = logits.double()
        nll = torch.logsumexp(z, 1) - z.gather(1, y.unsqueeze(1)).squeeze(1)
        sums = torch.stack(((w.double() * nll)[valid].sum(), w.double()[valid].sum()))
        counts = torch.tensor([int(keep.sum()), int(bad.sum())], dtype=torch.int64)
        grad = None
        if want_grad:
            grad = ((torch.softmax(z, 1) - F.one_hot(y, c).double()) * w.double().unsqueeze(1)).float()
            grad[~valid] = 0.0
        return sums, counts, grad

    @staticmethod
    def masked_finish(sums, counts):
        a, b = sums[0], sums[1]
        inv = (1.0 / b).float() if int(counts[0] - counts[1]) > 0 else torch.zeros(())
        return torch.stack((a.float(), b.float(), (a / b).float(), inv))

    @staticmethod
    def confusion_counts(logits, target, mask, ignore_index):
        c = logits.size(1)
        keep = _SemiOps._selected(target, mask, ignore_index)
        bad = keep & ((target < 0) | (target >= c))
        valid = keep & ~bad
        buf = torch.zeros(c * c + 1, dtype=torch.int64)
        if logits.size(0):
            pred = torch.from_numpy(logits.detach().numpy().argmax(axis=1))
            buf[: c * c] = torch.bincount(target[valid] * c + pred[valid], minlength=c * c)
        buf[c * c] = int(bad.sum())
        return buf

    @staticmethod
    def _factors(rows, n, site):
        if site is None:
            return torch.ones(rows.numel())
        from pathpyg_amd.nn.sharded import dropout_mask_diagonal
        return dropout_mask_diagonal(rows, n, *site)

    @staticmethod
    def one_hot_forward(plan, wt, bias, rows, n, site, out):
        t = wt.detach()[rows] * _SemiOps._factors(rows, n, site).unsqueeze(1)
        out.copy_(CpuOps.spmm(plan.fwd_ptr, plan.fwd_idx, plan.fwd_val, plan.n_dst, t, plan.self_coef, t, bias.detach(), True))

    @staticmethod
    def one_hot_backward(plan, dpre, rows, n, site):
        g = CpuOps.spmm(plan.bwd_ptr, plan.bwd_idx, plan.bwd_val, plan.n_src, dpre)
        g[: plan.n_dst] += plan.self_coef.unsqueeze(1) * dpre
        g = g * _SemiOps._factors(rows, n, site).unsqueeze(1)
        return torch.zeros(n, dpre.size(1)).index_add_(0, rows, g)


class CpuOpsSemi(_SemiOps, CpuOps):
    name = "cpu-test-standin (semi-supervised)"


class CpuOpsNodeSemi(_SemiOps, CpuOpsNode):
    name = "cpu-test-standin (semi-supervised, node-range partition)"
