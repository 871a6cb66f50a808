#!/usr/bin/env python3
"""Time the random graph models of pathpyg_amd.algorithms.generative_models on the device and write profiles/generative.txt.

    python tools/bench_generative.py [--sizes 10000,100000,1000000,10000000] [--degree 10] [--repeats 3] [--out profiles/generative.txt]

G(n,p) (undirected, mean degree ``--degree``) is split into its passes — count, scan with its read-back, fill, mirror (concatenate and
coalesce) — and so is the block model with 10 and 100 equal blocks (inside a block four times the density of between blocks, same mean
degree).  G(n,m) with the same number of edges is split into draws, the selection of the first m distinct (sort, two scans, compaction),
decode and mirror.  Every figure is the median of ``--repeats`` runs after one warm-up, with the stream drained around every stage.
Reported: sampled edges per second end to end, and the fill pass's bytes per second at 16 bytes per stored edge (two int64 ends).  The
CPU yardstick is a vectorised numpy Bernoulli over all pairs (one float32 per pair of the lower triangle), where that fits in memory.
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

from pathpyg_amd import _dispatch, _hip  # noqa: E402
from pathpyg_amd.algorithms import generative_models as gm  # noqa: E402


class Stages:
    def __init__(self):
        self.t = {}
        self._t0 = 0.0

    def start(self):
        torch.cuda.synchronize()
        self._t0 = time.perf_counter()

    def stop(self, name):
        torch.cuda.synchronize()
        self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - self._t0


def mirror(edge_index, n):
    return _dispatch.coalesce(torch.cat((edge_index, edge_index.flip(0)), dim=1), None, n)[0]


def run_regions(regions, n, seed, dev, perm=None):
    st = Stages()
    rows, n_chunks = gm.region_table(regions)
    table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 8).to(dev)
    st.start()
    counts = _hip.rg_region_count(table, n_chunks, seed)
    st.stop("count")
    st.start()
    offsets = _hip.exclusive_scan(counts)
    total = int(offsets[-1].item())
    st.stop("scan")
    st.start()
    ei = _hip.rg_region_fill(table, n_chunks, seed, offsets, total, n, perm)
    st.stop("fill")
    st.start()
    stored = mirror(ei, n)
    st.stop("mirror")
    return total, stored.size(1), st.t


def run_gnp(n, degree, seed, dev):
    N, kind, cols = gm.slot_space(n, False, False)
    return run_regions([(N, degree / (n - 1), kind, cols, 0, 0)], n, seed, dev)


def run_sbm(n, degree, blocks, seed, dev):
    # inside a block four times the density of between blocks; mean degree as asked
    size = n // blocks
    between = degree / ((n - size) + 4.0 * (size - 1))
    M = np.full((blocks, blocks), between)
    np.fill_diagonal(M, min(4.0 * between, 1.0))
    z = torch.arange(n, dtype=torch.int64, device=dev) % blocks
    st = Stages()
    st.start()
    sizes, perm = _dispatch.random_block_order(z, blocks, device=dev)
    st.stop("order")
    total, stored, t = run_regions(gm.block_regions(M, sizes), n, seed, dev, perm)
    t["order"] = st.t["order"]
    return total, stored, t


def run_gnm(n, degree, seed, dev):
    m = n * degree // 2
    N, kind, cols = gm.slot_space(n, False, False)
    st = Stages()
    batch = gm.gnm_first_batch(N, m)
    st.start()
    values = _dispatch.random_draws(N, seed, 0, batch, device=dev)
    st.stop("draws")
    st.start()
    distinct, slots = _dispatch.random_first_distinct(values, m, N.bit_length())
    st.stop("select")
    if slots is None:                                                   # (four deviations short: not expected; the public function would extend the batch)
        raise RuntimeError(f"{batch} draws gave only {distinct} of {m} distinct slots")
    st.start()
    ei = _dispatch.random_decode(slots, kind, cols)
    st.stop("decode")
    st.start()
    stored = mirror(ei, n)
    st.stop("mirror")
    return m, stored.size(1), st.t


def numpy_yardstick(n, degree):
    p = degree / (n - 1)
    rng = np.random.default_rng(1)
    t0 = time.perf_counter()
    edges = 0
    for lo in range(0, n, 4096):                                        # rows in blocks: one float32 per pair at or below the diagonal block
        hi = min(n, lo + 4096)
        hit = rng.random((hi - lo, hi), dtype=np.float32) < p
        r, c = np.nonzero(hit)
        edges += int((c < r + lo).sum())
    return edges, time.perf_counter() - t0


def median_of(fn, repeats):
    fn()                                                                # warm-up: allocator, code objects
    runs = [fn() for _ in range(repeats)]
    names = list(runs[0][2])
    return runs[0][0], runs[0][1], {k: statistics.median(r[2][k] for r in runs) for k in names}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="10000,100000,1000000,10000000")
    ap.add_argument("--degree", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-max", type=int, default=30000, help="largest n for the all-pairs numpy yardstick")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "generative.txt"))
    ap.add_argument("--chunk-edges", type=int, default=None, help="expected edges per chunk (default: the module's CHUNK_EDGES)")
    args = ap.parse_args()
    if args.chunk_edges:
        gm.CHUNK_EDGES = args.chunk_edges
    dev = _dispatch.compute_device()
    lines = [f"# tools/bench_generative.py: mean degree {args.degree}, medians of {args.repeats} after one warm-up, milliseconds per stage",
             f"# device: {torch.cuda.get_device_name(dev)}; CHUNK_EDGES = {gm.CHUNK_EDGES}; fill bytes = 16 per sampled edge",
             "# model            n   sampled edges  stored edges | stages (ms) | total ms | edges/s | fill GB/s"]

    def report(name, n, result):
        total, stored, t = result
        whole = sum(t.values())
        stages = "  ".join(f"{k} {v * 1e3:.3f}" for k, v in t.items())
        fill = f"{16.0 * total / t['fill'] / 1e9:.1f}" if "fill" in t and t["fill"] > 0 else "-"
        line = f"{name:<12} {n:>9} {total:>12} {stored:>12} | {stages} | {whole * 1e3:.3f} | {total / whole:.3e} | {fill}"
        print(line, flush=True)
        lines.append(line)

    for n in [int(x) for x in args.sizes.split(",")]:
        report("gnp", n, median_of(lambda: run_gnp(n, args.degree, 7, dev), args.repeats))
        report("gnm", n, median_of(lambda: run_gnm(n, args.degree, 7, dev), args.repeats))
        for blocks in (10, 100):
            report(f"sbm{blocks}", n, median_of(lambda: run_sbm(n, args.degree, blocks, 7, dev), args.repeats))
        if n <= args.numpy_max:
            edges, seconds = numpy_yardstick(n, args.degree)
            line = f"{'numpy pairs':<12} {n:>9} {edges:>12} {'-':>12} | host, all pairs, float32 | {seconds * 1e3:.3f} | {edges / seconds:.3e} | -"
            print(line, flush=True)
            lines.append(line)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
