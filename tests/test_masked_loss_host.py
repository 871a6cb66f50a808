"""Host side of the masked loss: the torch form that CPU tensors (and everything the kernel does not take) run, the node split, and the
unchanged default call.  No GPU."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

import pathpyg_amd as pp


def _case(n=101, c=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    z, y = torch.randn(n, c, generator=g), torch.randint(0, c, (n,), generator=g)
    return z, y, torch.rand(n, generator=g) < 0.4, 0.5 + torch.rand(c, generator=g)


@pytest.mark.parametrize("reduction", ("mean", "sum"))
@pytest.mark.parametrize("weighted", (False, True))
def test_cpu_tensors_run_the_gather_form(reduction, weighted):
    z, y, mask, w = _case()
    w = w if weighted else None
    y[~mask] = -1                                              # unlabelled nodes
    leaf, ref = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    got = pp.nn.cross_entropy(leaf, y, mask=mask, weight=w, reduction=reduction)
    want = F.cross_entropy(ref[mask], y[mask], weight=w, reduction=reduction)
    got.backward()
    want.backward()
    assert torch.equal(got, want) and torch.equal(leaf.grad, ref.grad) and bool((leaf.grad[~mask] == 0).all())


def test_ignore_index_equals_masking_and_an_empty_selection_is_nan_with_zero_gradient():
    z, y, mask, w = _case(seed=1)
    hidden = y.clone()
    hidden[~mask] = -1
    a = pp.nn.cross_entropy(z, hidden, ignore_index=-1, weight=w)
    b = pp.nn.cross_entropy(z, y, mask=mask, weight=w)
    torch.testing.assert_close(a, b, rtol=1e-6, atol=0)
    leaf = z.clone().requires_grad_(True)
    loss = pp.nn.cross_entropy(leaf, y, mask=torch.zeros_like(mask))
    loss.backward()
    assert math.isnan(float(loss.detach())) and bool((leaf.grad == 0).all())
    with pytest.raises(ValueError):
        pp.nn.cross_entropy(z, y, mask=mask, reduction="none")


def test_default_call_is_unchanged():
    params = inspect.signature(pp.nn.cross_entropy).parameters
    assert list(params)[:2] == ["logits", "target"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in params.items() if name not in ("logits", "target"))
    assert {n: p.default for n, p in params.items() if p.kind is inspect.Parameter.KEYWORD_ONLY} == dict(
        mask=None, weight=None, ignore_index=None, reduction="mean")
    z, y, _, _ = _case(seed=2)
    assert torch.equal(pp.nn.cross_entropy(z, y), F.cross_entropy(z, y))
    y[3] = -100                                                # torch's default ignore_index still goes through torch
    assert torch.equal(pp.nn.cross_entropy(z, y), F.cross_entropy(z, y))


def test_evaluate_on_cpu_tensors():
    z = torch.tensor([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [float("nan"), 5.0, 0.0], [0.0, 0.0, 3.0], [9.0, 0.0, 0.0]])
    y = torch.tensor([0, 2, 0, 2, 7])
    res = pp.nn.evaluate(z, y, mask=torch.tensor([True, True, True, True, False]))
    assert res["confusion"].tolist() == [[2, 0, 0], [0, 0, 0], [0, 1, 1]]          # ties to the lowest class, the NaN is the maximum
    assert res["support"].tolist() == [2, 0, 2] and res["accuracy"] == 0.75 and res["balanced_accuracy"] == 0.75
    assert abs(res["macro_f1"] - (1.0 + 0.0 + 2 / 3) / 3) <= 1e-12
    with pytest.raises(IndexError):
        pp.nn.evaluate(z, y)


@pytest.mark.parametrize("num_val,num_test,sizes", [(0.5, 0, (51, 50, 0)), (0.25, 0.1, (66, 25, 10)), (7, 3, (91, 7, 3)), (0, 0, (101, 0, 0))])
def test_random_node_split(num_val, num_test, sizes):
    data = pp.Data(x=torch.zeros(101, 2), y=torch.zeros(101, dtype=torch.int64))
    out = pp.utils.random_node_split(data, num_val=num_val, num_test=num_test, generator=torch.Generator().manual_seed(3))
    assert out is data
    masks = (data.train_mask, data.val_mask, data.test_mask)
    assert all(m.dtype == torch.bool and tuple(m.shape) == (101,) and m.device == data.y.device for m in masks)
    assert tuple(int(m.sum()) for m in masks) == sizes
    assert bool((sum(m.to(torch.int64) for m in masks) == 1).all())               # disjoint, and every node is somewhere
    again = pp.utils.random_node_split(pp.Data(x=torch.zeros(101, 2)), num_val=num_val, num_test=num_test,
                                       generator=torch.Generator().manual_seed(3))
    assert all(torch.equal(a, b) for a, b in zip(masks, (again.train_mask, again.val_mask, again.test_mask)))
    other = pp.utils.random_node_split(pp.Data(x=torch.zeros(101, 2)), num_val=num_val, num_test=num_test,
                                       generator=torch.Generator().manual_seed(4))
    assert sizes[0] == 101 or not torch.equal(other.train_mask, data.train_mask)


def test_random_node_split_rejects_other_splits_and_too_many_nodes():
    data = pp.Data(x=torch.zeros(10, 2))
    with pytest.raises(ValueError):
        pp.utils.random_node_split(data, split="random")
    with pytest.raises(ValueError):
        pp.utils.random_node_split(data, num_val=8, num_test=3)
