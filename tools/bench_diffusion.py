#!/usr/bin/env python3
"""The batched propagator (csrc/pp_graph_diffusion.hip) on directed G(n,p) graphs of mean degree 10.

    python tools/bench_diffusion.py [--out profiles/diffusion.txt] [--sizes 100000,1000000]

Printed per size:

* the time PER ITERATION of the walk mode for B = 1, 16 and 64 columns, from two runs of the dispatch function with a negative threshold
  (exactly 16 and 80 iterations): (t80 - t16) / 64, which leaves out the set-up, the staging of the block and the result; and over that time
  the bytes one iteration must move — per entry its source index and probability (16) and the B gathered doubles, per node the pointer (8),
  the dangling flag (1) and the B doubles read and written — as a bandwidth, and the time per column;
* one run of B = 16 next to 16 runs of B = 1 (50 iterations each through the dispatch function, blocks resident on the device, host clock
  around a device synchronise, structure built before), and whether the columns have the same bits;
* ``pagerank`` end to end (graph resident on the device, pull structure built before, result as a device tensor) with its iteration count,
  and ``personalized_pagerank`` with 16 seeds next to 16 single calls;
* where networkx imports and the graph has at most --networkx-limit nodes, ``networkx.pagerank`` on the host for context (graph copy apart),
  and the largest difference of the values.

No threshold is attached to any time."""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _dispatch  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats: int):
    out, times = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def moved_bytes(n: int, k: int, B: int) -> int:
    return k * (16 + 8 * B) + n * (9 + 16 * B)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--degree", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--networkx-limit", type=int, default=100000)
    ap.add_argument("--out", default="profiles/diffusion.txt")
    args = ap.parse_args()
    try:
        import networkx as nx
    except ImportError:
        nx = None
    rank_mod = pp.algorithms.ranking
    med = statistics.median
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# tools/bench_diffusion.py: the batched propagator on directed G(n,p), mean degree {args.degree:g}; {torch.cuda.get_device_name(0)}; "
            f"--sizes {args.sizes} --repeats {args.repeats}; times in ms unless stated")
        warm = pp.algorithms.generative_models.erdos_renyi_gnp(200, 0.05, directed=True, seed=1, device=DEV)    # first launches load the code objects
        rank_mod.pagerank(warm), rank_mod.personalized_pagerank(warm, torch.arange(16)), pp.processes.RandomWalk(warm).evolve("weighted", 3)
        for size in args.sizes.split(","):
            n = int(size)
            g = pp.algorithms.generative_models.erdos_renyi_gnp(n, args.degree / (n - 1), directed=True, seed=0, device=DEV)
            rw = pp.processes.RandomWalk(g)
            col_ptr, src, table = rw.structure()                        # built once per graph, outside the timed calls
            k = src.numel()
            deg = col_ptr[1:] - col_ptr[:-1]
            say(f"== n = {g.n} nodes, k = {k} entries, largest in-degree {int(deg.max())}, {int(table.dangling.sum())} dangling nodes")
            gen = torch.Generator().manual_seed(0)
            per_iter = {}
            for B in (1, 16, 64):
                block = torch.rand((g.n, B), generator=gen, dtype=torch.float64).to(DEV)
                fixed = lambda it: _dispatch.graph_diffusion(rw.structure(), g.n, _dispatch.DIFFUSION_WALK, block, -1.0, it)  # noqa: E731
                fixed(16)
                _, t16 = timed(lambda: fixed(16), args.repeats)
                _, t80 = timed(lambda: fixed(80), args.repeats)
                per_iter[B] = (med(t80) - med(t16)) / 64
                moved = moved_bytes(g.n, k, B)
                say(f"  walk mode, B = {B:2d}: per iteration {per_iter[B] * 1e3:9.2f} us  ({per_iter[B] * 1e3 / B:8.2f} us per column)   "
                    f"{moved / 1e6:9.2f} MB -> {moved / (per_iter[B] * 1e-3) / 1e9:8.1f} GB/s")
            block = torch.rand((g.n, 16), generator=gen, dtype=torch.float64).to(DEV)
            evolve = lambda x: _dispatch.graph_diffusion(rw.structure(), g.n, _dispatch.DIFFUSION_WALK, x, -1.0, 50).final  # noqa: E731
            columns = [block[:, c:c + 1].contiguous() for c in range(16)]
            got, t_batch = timed(lambda: evolve(block), args.repeats)
            ones, t_single = timed(lambda: [evolve(x) for x in columns], args.repeats)
            same = all(torch.equal(got[:, c], ones[c][:, 0]) for c in range(16))
            say(f"  evolve, 50 steps: one run of B = 16 median {med(t_batch):9.3f}  min {min(t_batch):9.3f}   16 runs of B = 1 median "
                f"{med(t_single):9.3f}  min {min(t_single):9.3f}   ratio {med(t_single) / med(t_batch):5.2f}   columns bit-equal: {same}")
            rank, ts = timed(lambda: rank_mod.pagerank(g, return_tensor=True), args.repeats)
            uniform = torch.full((g.n, 1), 1.0 / g.n, dtype=torch.float64)
            iters = rank_mod._pagerank_block(g, 0.85, uniform, uniform, uniform, 100, 1e-06, None).iterations[0]
            say(f"  pagerank: call median {med(ts):9.3f}  min {min(ts):9.3f}  max {max(ts):9.3f}  ({iters} iterations)")
            seeds = torch.arange(16) * (g.n // 16)
            _, t_ppr = timed(lambda: rank_mod.personalized_pagerank(g, seeds), args.repeats)
            _, t_one = timed(lambda: [rank_mod.personalized_pagerank(g, seeds[c:c + 1]) for c in range(16)], args.repeats)
            say(f"  personalized_pagerank, 16 seeds: one call median {med(t_ppr):9.3f}   16 calls of one seed median {med(t_one):9.3f}   "
                f"ratio {med(t_one) / med(t_ppr):5.2f}")
            if nx is None:
                say("  reference route: networkx does not import here")
                continue
            if g.n > args.networkx_limit:
                say(f"  reference route: skipped above --networkx-limit {args.networkx_limit} nodes")
                continue
            t0 = time.perf_counter()
            nxg = nx.DiGraph()
            nxg.add_nodes_from(range(g.n))
            nxg.add_edges_from(g.data.edge_index.cpu().T.tolist())
            t_copy = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want = nx.pagerank(nxg)
            t_nx = (time.perf_counter() - t0) * 1e3
            want = np.array([want[v] for v in range(g.n)])
            worst = float(np.max(np.abs(rank.cpu().numpy() - want) / (np.abs(want) + np.sqrt(np.mean(want * want)))))
            say(f"  reference route, host: networkx.pagerank {t_nx:10.2f} ms + {t_copy:.2f} ms graph copy (one run; largest difference "
                f"{worst:.2e} of |value| + rms)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
