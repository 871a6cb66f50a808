"""Node splits for semi-supervised training (``torch_geometric.transforms.RandomNodeSplit``; PyG is not a dependency)."""
from __future__ import annotations

import torch


def _count(value, num_nodes: int, name: str) -> int:
    count = round(num_nodes * value) if isinstance(value, float) else int(value)
    if count < 0:
        raise ValueError(f"random_node_split: {name} must not be negative")
    return count


def random_node_split(data, split: str = "train_rest", num_val=0.5, num_test=0, generator: torch.Generator | None = None):
    """Sets the bool masks ``train_mask`` / ``val_mask`` / ``test_mask`` [num_nodes] on ``data`` (on ``data.y``'s device; without labels,
    ``data.x``'s) and returns it: ``num_val`` validation and ``num_test`` test nodes drawn from one random permutation, every other node
    for training — PyG's ``RandomNodeSplit(split="train_rest")``, the split of the reference's tutorial loop.  A float is a fraction,
    rounded with ``round(num_nodes * f)``; an int is a count.  The three masks are disjoint and cover every node.  ``generator``: a
    (CPU) ``torch.Generator`` for a reproducible split.  The masks go straight into ``pathpyg_amd.nn.cross_entropy(out, y, mask=...)``
    and ``pathpyg_amd.nn.evaluate``."""
    if split != "train_rest":
        raise ValueError(f"random_node_split: only split='train_rest' is supported, got {split!r}")
    n = data.num_nodes
    if n is None:
        raise ValueError("random_node_split: data has no num_nodes")
    n = int(n)
    n_val, n_test = _count(num_val, n, "num_val"), _count(num_test, n, "num_test")
    if n_val + n_test > n:
        raise ValueError(f"random_node_split: num_val + num_test = {n_val + n_test} exceeds the {n} nodes")
    perm = torch.randperm(n, generator=generator)
    where = torch.zeros(n, dtype=torch.int8)                  # 0 train, 1 validation, 2 test
    where[perm[:n_val]] = 1
    where[perm[n_val: n_val + n_test]] = 2
    anchor = getattr(data, "y", None)
    if not isinstance(anchor, torch.Tensor):
        anchor = getattr(data, "x", None)
    device = anchor.device if isinstance(anchor, torch.Tensor) else torch.device("cpu")
    data.train_mask, data.val_mask, data.test_mask = ((where == k).to(device) for k in range(3))
    return data
