#!/usr/bin/env python3
"""Time the degree-sequence models of pathpyg_amd.algorithms.generative_models on the device and write profiles/degree_models.txt.

    python tools/bench_degree_models.py [--n 1000000] [--k 10] [--repeats 3] [--python-limit 2000] [--reference <src dir>] [--out ...]

Three items: ``k_regular_random(k, n)``, ``molloy_reed`` of a heavy-tailed graphic sequence of n nodes (Zipf with exponent 2.5, capped at
1000, parity mended on the first node) and ``is_graphic_erdos_gallai`` of that sequence.  The sampler is timed in its stages — the test
for graphicness, the first matching (stub keys, sort, pairing), the repair rounds, the mirror-and-sort into the stored graph — with the
stream drained around each, and once more as the public call end to end; every figure is the median of ``--repeats`` runs after one
warm-up.  Reported: milliseconds, repair rounds, sampled edges per second.  Where the reference package imports (``--reference`` names
the directory that holds ``pathpyG``), its own functions are timed on the host at ``--python-limit`` nodes: its loops are quadratic.
There is no acceptance threshold on any of these times.
"""
from __future__ import annotations

import argparse
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pathpyg_amd import _dispatch  # noqa: E402
from pathpyg_amd.algorithms import generative_models as gm  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def heavy_tailed(n: int, seed: int = 1) -> np.ndarray:
    s = np.minimum(np.random.default_rng(seed).zipf(2.5, size=n), 1000).astype(np.int64)
    s[0] += int(s.sum() & 1)
    return s


def run_sampler(degrees: torch.Tensor, seed: int):
    """``(edges, rounds, {stage: seconds})`` of the stages of ``molloy_reed`` on a device-resident int64 degree vector."""
    n, t = degrees.numel(), {}
    graphic, t["graphic"] = clock(lambda: _dispatch.random_graphic(degrees))
    if not graphic:
        raise RuntimeError("the benchmark's sequence is not graphic")
    (edge_index, _), t["matching"] = clock(lambda: _dispatch.random_matching(degrees, n, seed, False, True, gm.MAX_REPAIR_ROUNDS))
    (edge_index, rounds), whole = clock(lambda: _dispatch.random_matching(degrees, n, seed, False, False, gm.MAX_REPAIR_ROUNDS))
    t["repair"] = max(whole - t["matching"], 0.0)                       # (the matching is made again: the rounds work in place)
    _, t["store"] = clock(lambda: gm._finish(edge_index, n, None, False, None, row_sorted=False))
    return edge_index.size(1), rounds, t


def median_of(fn, repeats):
    fn()                                                                # warm-up: allocator, code objects
    runs = [fn() for _ in range(repeats)]
    return runs[0][0], runs[0][1], {k: statistics.median(r[2][k] for r in runs) for k in runs[0][2]}


def reference_module(path: str | None):
    if path:
        sys.path.insert(0, path)
    try:
        from pathpyG.algorithms import generative_models as ref
        return ref
    except Exception as why:                                            # noqa: BLE001 - any failure to import means: no yardstick
        print(f"# the reference does not import ({type(why).__name__}): no host yardstick", flush=True)
        return None


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--python-limit", type=int, default=2000, help="nodes at which the reference's host functions are timed")
    ap.add_argument("--reference", default=None, help="directory that holds the reference's pathpyG package")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "degree_models.txt"))
    args = ap.parse_args()
    dev = _dispatch.compute_device()
    lines = [f"# tools/bench_degree_models.py: medians of {args.repeats} after one warm-up, milliseconds; device: {torch.cuda.get_device_name(dev)}",
             "# item                     n        edges  rounds | stages (ms) | total ms | edges/s"]

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    def report(name, n, edges, rounds, t):
        whole = sum(t.values())
        stages = "  ".join(f"{k} {v * 1e3:.3f}" for k, v in t.items())
        emit(f"{name:<20} {n:>9} {edges:>12} {rounds:>7} | {stages} | {whole * 1e3:.3f} | {edges / whole:.3e}")

    sequences = {f"k_regular k={args.k}": np.full(args.n, args.k, dtype=np.int64), "heavy-tailed": heavy_tailed(args.n)}
    for name, seq in sequences.items():
        d = torch.from_numpy(seq).to(dev)
        report(name, args.n, *median_of(lambda: run_sampler(d, 7), args.repeats))

        def public():
            g, seconds = clock(lambda: gm.k_regular_random(args.k, args.n, seed=7) if name.startswith("k_regular") else gm.molloy_reed(seq, seed=7))
            return g.m, gm.last_repair_rounds, {"public call, host sequence, node IDs": seconds}
        report(name + " (call)", args.n, *median_of(public, args.repeats))
    heavy = sequences["heavy-tailed"]
    for label, arg in (("device input", torch.from_numpy(heavy).to(dev)), ("host input", heavy)):
        def check():
            answer, seconds = clock(lambda: gm.is_graphic_erdos_gallai(arg))
            return int(answer), 0, {label: seconds}
        answer, _, t = median_of(check, args.repeats)
        emit(f"{'is_graphic':<20} {args.n:>9} {'-':>12} {'-':>7} | {label} {t[label] * 1e3:.3f} | {t[label] * 1e3:.3f} | answer {bool(answer)}; {args.n / t[label]:.3e} entries/s")

    ref = reference_module(args.reference)
    if ref is not None:
        m = args.python_limit
        small = heavy_tailed(m)
        for name, fn in (("ref is_graphic", lambda: ref.is_graphic_erdos_gallai(small.tolist())),
                         ("ref k_regular", lambda: ref.k_regular_random(args.k, m)),
                         ("ref molloy_reed", lambda: ref.molloy_reed(small.tolist()))):
            t0 = time.perf_counter()
            out = fn()
            seconds = time.perf_counter() - t0
            edges = out.m if hasattr(out, "m") else 0
            emit(f"{name:<20} {m:>9} {edges:>12} {'-':>7} | host, reference | {seconds * 1e3:.3f} | {(edges or m) / seconds:.3e}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
