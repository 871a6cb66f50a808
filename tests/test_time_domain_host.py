"""The ground the GPU timestamp-domain tests (test_gpu_time_domain.py) stand on, pinned on the CPU so that none of them can pass
vacuously: the shared streams hold what they claim (every special value, NaNs of both signs, descents), the expected event graphs are
non-empty where they should be, hit the window boundary exactly, reach the +inf events, and never start at a NaN or a -inf event; the
pair counts of the pool stream are fixed numbers; the vectorised oracle agrees with the mask loop where it is specified (finite times)
and the golden fixture made from the reference's own source agrees with the mask loop."""
import pathlib

import numpy as np
import pytest
import torch

from tests import time_domain_cases as tc

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "time_domain_vectors.npz"

# pairs of the time-sorted pool stream (seed 7, 900 events, 6 nodes) per delta
POOL_PAIRS = {5e-324: 993, 1.0: 6134, 2.0: 9978, 2.0 ** 53: 14855, 1.7e308: 38820, tc.INF: 46327}


def test_pool_stream_holds_every_special_value_and_is_unsorted():
    ei, t, n = tc.pool_stream()
    assert ei.shape == (2, 900) and t.dtype == torch.float64 and n == 6
    have = set(tc.bits(t).tolist())
    for v in tc.special_pool():
        assert int(np.array([v]).view(np.int64)[0]) in have, repr(v)
    perm = tc.torch_order(t)
    nan_at = torch.nonzero(torch.isnan(t)).flatten()
    assert nan_at.numel() > 0
    nan_bits = set(tc.bits(t[nan_at]).tolist())
    assert nan_bits == {0x7FF8000000000000, 0xFFF8000000000001 - (1 << 64)}              # both signs occur
    assert torch.equal(perm[-nan_at.numel():], nan_at)                                   # all NaNs last, in input order
    assert not torch.isnan(t[perm[:-nan_at.numel()]]).any()
    assert not torch.equal(perm, torch.arange(t.numel()))                                # the raw stream has descents
    st = t[perm]
    zeros = torch.nonzero(st == 0).flatten()
    signs = torch.signbit(st[zeros])
    assert signs.any() and not signs.all() and bool((signs[1:] != signs[:-1]).any())     # -0.0 and 0.0 tie: both signs, interleaved by input order


@pytest.mark.parametrize("name", ["pool", "mixed"])
def test_mixed_and_pool_streams_cover_the_kernel_paths(name):
    ei, t, n, perm = tc.stream(name)
    m = t.numel()
    assert m == (900 if name == "pool" else 4200)
    assert torch.isnan(t).any() and torch.isinf(t).any()
    if name == "mixed":
        assert m > 4096 and (m + 63) // 64 == 66                       # more than one sort tile, 66 waves of the count kernel
        special = ~torch.isfinite(t) | (t.abs() > 1e6) | ((t.abs() < 1e-300) & (t != 0))
        assert 0.02 * m < int(special.sum()) < 0.05 * m
        assert bool(torch.isnan(t[(m - 1) // 64 * 64]))                # the last wave starts at a NaN
        assert bool(torch.isinf(t[0])) and t[0] < 0                    # the first one at -inf


@pytest.mark.parametrize("d", tc.POSITIVE_DELTAS, ids=repr)
def test_positive_deltas_give_pairs_at_the_exact_boundary(d):
    ei, t, _, _ = tc.stream("pool")
    out = tc.expected_lift("pool", d)
    assert out.size(1) > 0
    if d in POOL_PAIRS:
        assert out.size(1) == POOL_PAIRS[d]
    ti, tj = t[out[0]], t[out[1]]
    assert bool((tj > ti).all()) and bool((tj <= ti + d).all())
    assert not torch.isnan(ti).any() and not torch.isnan(tj).any() and not (ti == -tc.INF).any()
    if d == 0.25:
        # no two pool values are 0.25 apart and no sum t + 0.25 rounds onto a LARGER pool value: the exact hit of this delta comes from
        # the mixed stream (times on a 0.01 grid)
        eim, tm, _, _ = tc.stream("mixed")
        outm = tc.expected_lift("mixed", d)
        assert bool((tm[outm[1]] == tm[outm[0]] + d).any())
    else:
        assert bool((tj == ti + d).any())
    if d in (1.7e308, tc.INF):
        assert bool((tj == tc.INF).any())


@pytest.mark.parametrize("name", ["pool", "mixed"])
@pytest.mark.parametrize("d", tc.EMPTY_DELTAS, ids=repr)
def test_zero_negative_and_nan_deltas_give_no_pair(name, d):
    assert tc.expected_lift(name, d).shape == (2, 0)


@pytest.mark.parametrize("d", tc.DELTAS, ids=repr)
def test_no_pair_starts_at_a_nan_or_minus_inf_event(d):
    for name in ("pool", "mixed"):
        _, t, _, _ = tc.stream(name)
        out = tc.expected_lift(name, d)
        ti = t[out[0]]
        assert not torch.isnan(ti).any() and not (ti == -tc.INF).any()
        assert not torch.isnan(t[out[1]]).any()


def test_python_float_and_int_deltas_are_the_tensor_deltas():
    ei, t, _, _ = tc.stream("pool")
    assert torch.equal(tc.mask_loop(ei, t, 1.0), tc.expected_lift("pool", 1.0))
    assert torch.equal(tc.mask_loop(ei, t, 0.25), tc.expected_lift("pool", 0.25))
    assert torch.equal(tc.mask_loop(ei, t, 2), tc.expected_lift("pool", 2.0))


@pytest.mark.filterwarnings("ignore:To copy construct from a tensor")          # the oracle's torch.tensor(delta), as the reference writes it
def test_vectorised_oracle_equals_the_mask_loop_on_finite_times():
    """``temporal_lift_sorted`` (the oracle of the large lift tests, bench.py's CPU baseline) is specified for finite times and
    thresholds; there it agrees with the mask loop on every finite extreme of the pool."""
    from oracle.lift import temporal_lift_sorted
    ei, t, n, _ = tc.stream("pool")
    keep = torch.isfinite(t)
    fei, ft = ei[:, keep].contiguous(), t[keep].contiguous()
    assert 0 < ft.numel() < t.numel()
    for d in tc.DELTAS:
        if not np.isfinite(d):
            continue
        want = tc.mask_loop(fei, ft, tc.delta_tensor(d))
        got = temporal_lift_sorted(fei, ft, tc.delta_tensor(d), n)
        assert torch.equal(got, want), repr(d)
        assert (want.size(1) > 0) == (d > 0)


@pytest.mark.filterwarnings("ignore:To copy construct from a tensor")
def test_vectorised_oracle_is_not_the_reference_on_nan_thresholds():
    """Why the tests of this domain use the mask loop: ``torch.searchsorted`` ranks a NaN threshold above every time."""
    from oracle.lift import temporal_lift_sorted
    ei, t, n, _ = tc.stream("pool")
    assert not torch.equal(temporal_lift_sorted(ei, t, tc.delta_tensor(tc.INF), n), tc.expected_lift("pool", tc.INF))


def test_golden_time_domain_vectors_equal_the_mask_loop():
    golden = np.load(GOLDEN, allow_pickle=False)
    ei, t, n, _ = tc.stream("pool")
    names = {"pool_delta1": 1.0, "pool_delta2p53": 2.0 ** 53, "pool_deltainf": tc.INF, "pool_deltanan": tc.NAN}
    assert {k.split("/")[1] for k in golden.files} == set(names)
    for name, d in names.items():
        assert torch.equal(torch.from_numpy(golden[f"temporal/{name}/edge_index"]), ei)
        assert torch.equal(tc.bits(torch.from_numpy(golden[f"temporal/{name}/time"])), tc.bits(t))
        assert int(golden[f"temporal/{name}/num_nodes"]) == n and str(golden[f"temporal/{name}/delta_kind"]) == "float"
        gd = float(golden[f"temporal/{name}/delta"])
        assert gd == d or (np.isnan(gd) and np.isnan(d))
        out = torch.from_numpy(golden[f"temporal/{name}/out"]).long()
        assert (str(golden[f"temporal/{name}/raised"]) != "") == (out.size(1) == 0)
        key = out[0] * ei.size(1) + out[1]                       # the reference emits the pairs timestamp by timestamp
        assert torch.equal(out[:, torch.sort(key).indices], tc.expected_lift("pool", d)), name
    assert golden["temporal/pool_deltainf/out"].shape[1] == POOL_PAIRS[tc.INF]
    assert golden["temporal/pool_deltanan/out"].shape[1] == 0
