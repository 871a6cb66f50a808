"""CPU tests of the merged-weight semantics every GPU parity test is measured against: the oracle's PyG ``coalesce``
(oracle/aggregate.py) sums fp32 weights LEFT TO RIGHT, so a sum of ones stops at 2^24 and a fractional sum equals a plain
sequential float32 loop.  The builders keep that order below 2^24 and write exact counts beyond ("Merged weights")."""
import numpy as np
import torch

from oracle import aggregate as oa


def _one_pair(n_copies: int) -> torch.Tensor:
    ei = torch.zeros((2, n_copies + 1), dtype=torch.int64)
    ei[1, :n_copies] = 1
    ei[:, n_copies] = torch.tensor([1, 0])          # (a second, single edge)
    return ei


def test_a_sum_of_unit_weights_stops_at_2_24():
    n = (1 << 24) + 2
    index, weight = oa.coalesce(_one_pair(n), torch.ones(n + 1), 2)
    assert index.tolist() == [[0, 1], [1, 0]]
    assert weight.tolist() == [16777216.0, 1.0]
    assert float(np.float32(n)) == 16777218.0        # (what an exact count gives: the deviation the GPU tests accept)


def test_fractional_weights_are_summed_left_to_right():
    rng = np.random.default_rng(0)
    w = (rng.random(1000) + 0.25).astype(np.float32)
    acc = np.float32(0.0)
    for v in w:
        acc = np.float32(acc + v)
    _, weight = oa.coalesce(_one_pair(1000), torch.from_numpy(np.append(w, np.float32(2.5))), 2)
    assert weight[0].item() == float(acc)
    assert weight[1].item() == 2.5
    # the order is visible in the low bits: pairwise (numpy) and float64 summation give other values
    assert float(acc) != float(np.sum(w)) and float(acc) != float(np.float32(w.astype(np.float64).sum()))
