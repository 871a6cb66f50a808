#!/usr/bin/env python3
"""eigenvector_centrality and katz_centrality (csrc/pp_graph_power.hip) on seeded random digraphs.

    python tools/bench_spectral_centrality.py [--out profiles/spectral_centrality.txt] [--sizes 5000:50000,100000:2000000,1000000:20000000]

Each size is ``nodes:edges`` (uniform random ends; parallel edges collapse, so the structure has slightly fewer entries).  Printed per size
and measure, unit and weighted: the end-to-end time of the public call (host clock around a device synchronise, graph resident on the
device, predecessor structure built before, result as a device tensor) with its iteration count, and the time PER ITERATION from two runs of
the dispatch function that cannot converge (threshold 0) with 16 and 80 iterations: (t80 - t16) / 64, which leaves out the set-up and the
result.  From the bytes one iteration must move — 16 per entry (index, gathered value; 8 more when weighted) and 24 per node (eigenvector:
40, its scale pass reads and writes the vector once more) — the achieved bandwidth.  Where networkx imports and the graph has at most
--networkx-limit nodes, the same call through a ``DiGraph`` copy is timed on the host, copy included, and the values are compared.
No threshold is attached to any time."""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _dispatch, _hip  # noqa: E402

DEV = "cuda:0"
ALPHA = 0.02


def random_graph(nodes: int, edges: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, nodes, (2, edges), generator=g)
    w = torch.rand(edges, generator=g, dtype=torch.float64) + 0.5
    return pp.Graph(pp.Data(edge_index=ei.to(DEV), edge_weight=w.to(DEV), num_nodes=nodes))


def timed(fn, repeats: int):
    out, times = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000:50000,100000:2000000,1000000:20000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--networkx-limit", type=int, default=20000)
    ap.add_argument("--out", default="profiles/spectral_centrality.txt")
    args = ap.parse_args()
    try:
        import networkx as nx
    except ImportError:
        nx = None
    cen = pp.algorithms.centrality
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# tools/bench_spectral_centrality.py: power-iteration centralities on uniform random digraphs; {torch.cuda.get_device_name(0)}; "
            f"--sizes {args.sizes} --repeats {args.repeats}; katz alpha {ALPHA}; times in ms")
        warm = random_graph(50, 300, seed=1)                        # first launches load the code objects: not part of any number below
        cen.eigenvector_centrality(warm), cen.katz_centrality(warm, ALPHA, weight="edge_weight")
        for size in args.sizes.split(","):
            nodes, edges = (int(x) for x in size.split(":"))
            g = random_graph(nodes, edges)
            col_ptr, _, _ = g.simple_predecessors()                  # built once per graph, outside the timed calls
            n, k = g.n, g.simple_predecessors()[1].numel()
            deg = col_ptr[1:] - col_ptr[:-1]
            say(f"== n = {n} nodes, {edges} stored edges, k = {k} distinct entries, largest in-degree {int(deg.max())}")
            calls = {"eigenvector": lambda weight: cen.eigenvector_centrality(g, max_iter=1000, weight=weight, return_tensor=True),
                     "katz": lambda weight: cen.katz_centrality(g, ALPHA, weight=weight, return_tensor=True)}
            results = {}
            for name, fn in calls.items():
                for weight in (None, "edge_weight"):
                    label = f"{name}{' weighted' if weight else ''}"
                    results[label], ts = timed(lambda: fn(weight), args.repeats)
                    mode = _hip.POWER_EIGENVECTOR if name == "eigenvector" else _hip.POWER_KATZ
                    iters = _dispatch.graph_power_centrality(g, mode, n * 1e-06, 1000, alpha=ALPHA, beta=1.0, weight=weight)[1]   # the same call
                    fixed = lambda it: _dispatch.graph_power_centrality(g, mode, 0.0, it, alpha=ALPHA, beta=1.0, weight=weight)  # noqa: E731
                    _, t16 = timed(lambda: fixed(16), args.repeats)
                    _, t80 = timed(lambda: fixed(80), args.repeats)
                    per_iter = (statistics.median(t80) - statistics.median(t16)) / 64
                    moved = (24 if weight else 16) * k + (40 if name == "eigenvector" else 24) * n
                    say(f"  {label:<22s}: call median {statistics.median(ts):9.3f}  min {min(ts):9.3f}  max {max(ts):9.3f}  ({iters} iterations)   "
                        f"per iteration {per_iter * 1e3:9.2f} us   {moved / 1e6:9.2f} MB -> {moved / (per_iter * 1e-3) / 1e9:8.1f} GB/s")
            if nx is None:
                say("  reference route: networkx does not import here")
                continue
            if n > args.networkx_limit:
                say(f"  reference route: skipped above --networkx-limit {args.networkx_limit} nodes")
                continue
            ei = g.data.edge_index.cpu()
            t0 = time.perf_counter()
            nxg = nx.DiGraph()
            nxg.add_nodes_from(range(n))
            nxg.add_edges_from(ei.T.tolist())
            t_copy = (time.perf_counter() - t0) * 1e3
            for label, call in (("eigenvector", lambda: nx.eigenvector_centrality(nxg, max_iter=1000)),
                                ("katz", lambda: nx.katz_centrality(nxg, ALPHA))):
                t0 = time.perf_counter()
                want = call()
                t_nx = (time.perf_counter() - t0) * 1e3
                want = np.array([want[v] for v in range(n)])
                got = results[label].cpu().numpy()
                worst = float(np.max(np.abs(got - want) / (np.abs(want) + np.sqrt(np.mean(want * want)))))
                say(f"  reference route, host: networkx {label}_centrality {t_nx:10.2f} ms + {t_copy:.2f} ms graph copy (one run; largest "
                    f"difference {worst:.2e} of |value| + rms)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
