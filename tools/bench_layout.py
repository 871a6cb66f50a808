#!/usr/bin/env python3
"""The Fruchterman-Reingold layout (csrc/pp_graph_layout.hip) on seeded random sparse graphs with m = 5 n stored edges.

    python tools/bench_layout.py [--out profiles/layout.txt] [--sizes 1000,10000,100000] [--host-sizes 1000,5000]

GPU half, per size: the time PER ITERATION from two runs of the dispatch function that cannot stop early (threshold -1) with a few and with
many iterations, (t_many - t_few) / (many - few), which leaves out the set-up, the adjacency and the result (host clock around a device
synchronise, graph and start positions resident on the device, every shape warmed up first); from it the pair interactions per second,
n^2 per iteration, and what that is in fp64 vector instructions (18 per pair in the compiled inner loop, the division's 12 included)
against the 39.3 T/s at which the chip issues fp64 FMAs (78.6 TFLOPS).  Then the end-to-end time of the public call with its defaults
(50 iterations, adjacency, start draws and rescale included, result as a device tensor).
Host half, where networkx imports: ``networkx.spring_layout`` on the same graphs, 50 iterations (from 500 nodes on that is networkx's
float32 row loop), one run each; a size that does not finish within --host-limit seconds is reported as such.  The GPU half needs no
networkx; the host half needs no GPU (--skip-gpu).  No threshold is attached to any time."""
import argparse
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")

INSTRUCTIONS_PER_PAIR = 18          # v_*_f64 in the inner loop of k_layout_repulse per source (72 per 4), from the compiled ISA
FP64_ISSUE_RATE = 39.3e12           # fp64 vector instructions per second: 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz


def random_edges(n: int, seed: int = 0) -> torch.Tensor:
    return torch.randint(0, n, (2, 5 * n), generator=torch.Generator().manual_seed(seed))


def gpu_half(sizes, repeats, say):
    import pathpyg_amd as pp
    from pathpyg_amd import _dispatch

    dev = "cuda:0"

    def timed(fn):
        out, times = None, []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return out, times

    say(f"# GPU: {torch.cuda.get_device_name(0)}; float64; times in ms; {repeats} repeats, medians")
    for n in sizes:
        g = pp.Graph(pp.Data(edge_index=random_edges(n).to(dev), num_nodes=n))
        adjacency = _dispatch.graph_layout_adjacency(g)
        start = _dispatch.layout_start(1, n, 1.0, (0.0, 0.0), device=dev)
        k = float(np.sqrt(1.0 / n))
        few, many = (16, 80) if n <= 20000 else (2, 10)
        run = lambda its: _dispatch.graph_fr_layout(adjacency, start, k, None, None, its, -1.0, with_stats=True)  # noqa: E731
        _, ran, _, stats = run(few)                                     # warm-up of this shape
        assert ran == few
        _, t_few = timed(lambda: run(few))
        _, t_many = timed(lambda: run(many))
        per_iter = (statistics.median(t_many) - statistics.median(t_few)) / (many - few)
        pairs = n * n / (per_iter * 1e-3)
        say(f"== n = {n}, {5 * n} stored edges, {adjacency[1].numel()} adjacency entries; repulsion grid {stats.target_blocks} x {stats.chunks}, "
            f"attraction grid {stats.light_grid}")
        say(f"  per iteration {per_iter:10.4f} ms  ({few} iterations: {statistics.median(t_few):.3f}, {many}: {statistics.median(t_many):.3f})   "
            f"{pairs:.3e} pair interactions / s = {pairs * INSTRUCTIONS_PER_PAIR:.3e} fp64 instructions / s, "
            f"{100 * pairs * INSTRUCTIONS_PER_PAIR / FP64_ISSUE_RATE:.1f} % of the fp64 vector issue rate")
        pp.layout(g, "spring", seed=1, return_tensor=True)
        _, ts = timed(lambda: pp.layout(g, "spring", seed=1, return_tensor=True))
        say(f"  pp.layout(g, 'spring'), 50 iterations, end to end: median {statistics.median(ts):10.3f}  min {min(ts):10.3f}  max {max(ts):10.3f}  "
            f"({pp.visualisations.layout.last_iterations} iterations run)")


class _TooLong(Exception):
    pass


def host_half(sizes, limit, say):
    try:
        import networkx as nx
        import scipy.sparse as sp
    except ImportError:
        say("# host: networkx does not import here; not measured")
        return
    say(f"# host: networkx {nx.__version__} spring_layout, 50 iterations, one run each, limit {limit} s")

    def alarm(*_):
        raise _TooLong

    signal.signal(signal.SIGALRM, alarm)
    for n in sizes:
        ei = random_edges(n).numpy()
        G = nx.from_scipy_sparse_array(sp.coo_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n)))
        signal.alarm(limit)
        t0 = time.perf_counter()
        try:
            nx.spring_layout(G, seed=1)
            seconds = time.perf_counter() - t0
            say(f"== n = {n}: {seconds:.2f} s, {seconds / 50 * 1e3:.1f} ms per iteration, {n * n * 50 / seconds:.3e} pair interactions / s"
                f"{' (float32 row loop)' if n >= 500 else ''}")
        except _TooLong:
            say(f"== n = {n}: did not finish within {limit} s")
        finally:
            signal.alarm(0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--host-sizes", default="1000,5000")
    ap.add_argument("--host-limit", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-gpu", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default="profiles/layout.txt")
    args = ap.parse_args()
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# tools/bench_layout.py: Fruchterman-Reingold on uniform random graphs, m = 5 n; --sizes {args.sizes} --host-sizes {args.host_sizes}")
        if not args.skip_gpu:
            gpu_half([int(x) for x in args.sizes.split(",")], args.repeats, say)
        if not args.skip_host:
            host_half([int(x) for x in args.host_sizes.split(",")], args.host_limit, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
