"""CPU-side checks of the implicit one-hot features (no GPU): the deferred ``Identity`` of a ``Data`` bag and the torch statement of the
dropout factors of an identity's diagonal."""
import pickle

import pytest
import torch

from pathpyg_amd.data import Data, Identity, Lazy
from pathpyg_amd.nn.sharded import dropout_mask, dropout_mask_diagonal


def _unresolved(data, key="x"):
    held = data.peek(key)
    return isinstance(held, Identity) and held.value is None


def test_identity_stays_deferred_through_the_container_questions():
    data = Data(x=Identity(5, "cpu"), y=torch.arange(5))
    assert isinstance(data.peek("x"), Lazy) and _unresolved(data)
    assert data.peek("x").shape == (5, 5)
    assert data.num_nodes == 5 and data.is_node_attr("x") and not data.is_edge_attr("x")
    assert "x=[5, 5]" in repr(data)
    assert data.is_identity("x") and not data.is_identity("y") and not data.is_identity("absent")
    assert _unresolved(data)
    assert data.to("cpu") is data and _unresolved(data) and data.is_identity("x")
    copy = data.clone()
    assert _unresolved(copy) and copy.is_identity("x") and copy.peek("x") is not data.peek("x")
    assert _unresolved(data)


def test_identity_resolves_to_eye_and_is_recognised_until_replaced_or_edited():
    data = Data(x=Identity(5, "cpu"))
    x = data.x
    assert torch.equal(x, torch.eye(5)) and x.dtype == torch.float32
    assert data.peek("x") is x and data.x is x and data["x"] is x
    assert data.is_identity("x")
    # a copy of the made matrix is a tensor like any other; the original is untouched by it
    copy = data.clone()
    assert not copy.is_identity("x") and copy.peek("x") is not x and torch.equal(copy.x, torch.eye(5))
    assert data.is_identity("x")
    data.x.mul_(2)
    assert not data.is_identity("x")
    other = Data(x=Identity(5, "cpu"))
    other.x = torch.eye(5)
    assert not other.is_identity("x")                                   # an assigned tensor is just a tensor, whatever it holds
    late = Data(x=Identity(5, "cpu"))
    _ = late.x
    late.x = torch.eye(5)
    assert not late.is_identity("x")
    gone = Data(x=Identity(5, "cpu"))
    _ = gone.x
    del gone.x
    assert not gone.is_identity("x") and gone.x is None


def test_identity_pickles_as_its_size_and_device():
    data = Data(x=Identity(4096, "cpu"), num_nodes=4096)
    payload = pickle.dumps(data)
    assert len(payload) < 4096, len(payload)                            # (the matrix would be 4096 * 4096 * 4 bytes)
    back = pickle.loads(payload)
    assert _unresolved(back) and back.is_identity("x") and back.peek("x").shape == (4096, 4096) and back.peek("x").device == torch.device("cpu")
    assert _unresolved(data)
    assert len(pickle.dumps(Identity(4096, "cpu"))) < 4096
    # a resolved identity pickles as the tensor it became (the bag holds the tensor) and comes back as a plain tensor
    small = Data(x=Identity(3, "cpu"))
    _ = small.x
    again = pickle.loads(pickle.dumps(small))
    assert torch.equal(again.x, torch.eye(3)) and not again.is_identity("x")


def _picked_rows(n, count, seed):
    if n <= count:
        return torch.arange(n)
    g = torch.Generator().manual_seed(seed)
    low = torch.randint(0, min(n, 65_536), (count // 2 - 1,), generator=g)
    high = torch.randint(min(n - 1, 65_537), n, (count - count // 2 - 1,), generator=g)
    return torch.cat((torch.tensor([0, n - 1]), low, high))


@pytest.mark.parametrize("n", [7, 300, 70_001])
@pytest.mark.parametrize("p", [0.4, 0.0])
def test_dropout_mask_diagonal_is_the_diagonal_of_dropout_mask(n, p):
    rows = _picked_rows(n, 64, n)
    assert int(rows.min()) == 0 and int(rows.max()) == n - 1
    if n == 70_001:
        assert rows.numel() == 64 and int((rows > 65_536).sum()) >= 16
        assert int((rows * n + rows).max()) >= 2 ** 32                  # the high word of the hash index takes part
    for seed, tag in ((0, 0), (123456789, 64), (2 ** 31 - 2, 128)):
        full = dropout_mask(rows, n, p, seed, tag)
        want = full[torch.arange(rows.numel()), rows]
        got = dropout_mask_diagonal(rows, n, p, seed, tag)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    if p > 0:
        kept = dropout_mask_diagonal(torch.arange(n), n, p, 5, 0) > 0
        assert 0.5 < float(kept.float().mean()) < 0.7 if n >= 300 else kept.numel() == n       # about 1 - p of the diagonal survives
