"""Shared cases of the timestamp-domain tests (test_time_domain_host.py on the CPU, test_gpu_time_domain.py on the GPU): float64 event
times at the ends and in the holes of the number line — infinities, signed zeros, subnormals, neighbours beyond 2^53, NaNs of both signs —
and deltas whose thresholds ``t + delta`` saturate at inf or become NaN.

The expected event order is torch's (:func:`torch_order`): ascending, ``-0.0 == 0.0``, every NaN last and tied, stable.  The expected
event graph is the reference's mask loop (:func:`mask_loop`, ``oracle.lift.temporal_lift_per_timestamp``), the only oracle of this
package that holds on non-finite times: ``temporal_lift_sorted`` rests on ``torch.searchsorted``, which ranks a NaN threshold as the
largest value where the reference's ``<=`` is false.

No GPU is needed to import this module."""
from __future__ import annotations

import warnings

import numpy as np
import torch

INF = float("inf")
NAN = float("nan")


def _from_bits(bits: int) -> np.float64:
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


NAN_PLUS = _from_bits(0x7FF8000000000000)            # the quiet NaN of 0.0 / 0.0 on most machines ...
NAN_MINUS = _from_bits(0xFFF8000000000001)           # ... and one with the sign bit set (inf - inf on x86) and a payload


def special_pool() -> np.ndarray:
    return np.array([
        -INF, -1.7e308, -(2.0 ** 53) - 2, -(2.0 ** 53), -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308,
        1.0, 1.0 + 2.0 ** -52, 2.0, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 53 + 4, 1e300, 1.7e308, INF,
        NAN_PLUS, NAN_MINUS,
    ], dtype=np.float64)


def pool_stream(seed: int = 7, m: int = 900, n: int = 6):
    """``(edge_index [2, m] int64, time [m] float64, n)``: every time a pool value, UNSORTED."""
    pool = special_pool()
    rng = np.random.default_rng(seed)
    t = pool[rng.integers(0, len(pool), m)]
    ei = rng.integers(0, n, (2, m))
    return torch.from_numpy(ei), torch.from_numpy(t), n


def mixed_stream(seed: int, m: int = 4200, n: int = 40):
    """``(edge_index, time, n)``: normal times rounded to 2 decimals (ties, exact boundary hits for delta = 0.25), about 3 % of the
    positions overwritten with pool values and another 1 % with NaNs of alternating sign, UNSORTED.  More than one sort tile (4096 keys)
    and 66 waves of the count kernel; once sorted, wave 0 starts at a -inf event and the NaN tail is longer than the last wave
    (4200 - 4160 = 40 events), so that wave starts at a NaN and the one before holds the step from numbers over +inf to NaN."""
    pool = special_pool()
    rng = np.random.default_rng(seed)
    t = np.round(rng.normal(0, 50, m), 2)
    ei = rng.integers(0, n, (2, m))
    at = rng.choice(m, size=int(round(0.04 * m)), replace=False)
    k = int(round(0.03 * m))
    t[at[:k]] = pool[rng.integers(0, len(pool), k)]
    t[at[k:]] = np.where(np.arange(at.size - k) % 2 == 0, NAN_PLUS, NAN_MINUS)
    return torch.from_numpy(ei), torch.from_numpy(t), n


DELTAS = [0.0, 5e-324, 0.25, 1.0, 2.0, 2.0 ** 53, 1.7e308, INF, -1.0, -INF, NAN]
POSITIVE_DELTAS = [d for d in DELTAS if d > 0]
EMPTY_DELTAS = [0.0, -1.0, -INF, NAN]
DELTA_IDS = [repr(d) for d in DELTAS]


def delta_tensor(d: float) -> torch.Tensor:
    return torch.tensor(d, dtype=torch.float64)


def torch_order(t: torch.Tensor) -> torch.Tensor:
    """THE expected event order: the permutation of a stable ``torch.sort``."""
    return torch.sort(t, stable=True).indices


def sorted_stream(stream):
    """The stream in :func:`torch_order` + the permutation."""
    ei, t, n = stream
    perm = torch_order(t)
    return ei[:, perm].contiguous(), t[perm].contiguous(), n, perm


def weights(m: int, seed: int = 3) -> torch.Tensor:
    """Integer-valued float32 event weights in 1..4: merged sums are exact in any association."""
    return torch.from_numpy(np.random.default_rng(seed).integers(1, 5, m).astype(np.float32))


def mask_loop(ei: torch.Tensor, t: torch.Tensor, delta) -> torch.Tensor:
    """The reference's per-timestamp mask loop on CPU tensors; "no pair" (its ``torch.cat([])``) as an empty ``[2, 0]`` tensor, the pairs
    in lexicographic order."""
    from oracle.lift import temporal_lift_per_timestamp
    try:
        with warnings.catch_warnings():              # (the oracle's torch.tensor(delta), as the reference writes it, warns on a tensor delta)
            warnings.simplefilter("ignore", UserWarning)
            out = temporal_lift_per_timestamp(ei, t, delta)
    except (RuntimeError, ValueError):
        return torch.empty((2, 0), dtype=torch.long)
    key = out[0] * ei.size(1) + out[1]
    return out[:, torch.sort(key).indices].contiguous()


_STREAMS: dict = {}
_EXPECTED: dict = {}


def stream(name: str):
    """``(edge_index, time, n, perm)`` of the named stream in :func:`torch_order`; built once per process.  "pool": :func:`pool_stream`;
    "pool24": the same times over 24 nodes (no order-2 node with more than 4096 continuations at any delta, which is where the
    level-by-level builder hands a stream back); "mixed": :func:`mixed_stream` of seed 1."""
    if name not in _STREAMS:
        raw = {"pool": pool_stream, "pool24": lambda: pool_stream(n=24), "mixed": lambda: mixed_stream(1)}[name]()
        _STREAMS[name] = sorted_stream(raw)
    return _STREAMS[name]


def expected_lift(name: str, d: float) -> torch.Tensor:
    """:func:`mask_loop` of the named sorted stream for the float64 delta ``d``; computed once per process, never modified."""
    key = (name, repr(d))
    if key not in _EXPECTED:
        ei, t, _, _ = stream(name)
        _EXPECTED[key] = mask_loop(ei, t, delta_tensor(d))
    return _EXPECTED[key]


def bits(t: torch.Tensor) -> torch.Tensor:
    """float64 values as their int64 bit patterns: equality that tells NaN payloads and the signs of zero apart."""
    return t.contiguous().view(torch.int64)
