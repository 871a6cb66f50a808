#!/usr/bin/env python3
"""Colour refinement and the Weisfeiler-Leman test (csrc/pp_graph_wl.hip) on the aggregated static graph of the seeded temporal stream
tools/bench_static_paths.py uses (node = floor(nodes * u^3), u uniform: a few hubs far above one wave, most nodes with a handful of edges).

    python tools/bench_wl.py [--out profiles/wl.txt] [--sizes 5000:50000,100000:1000000,1000000:10000000]

Each size is ``nodes:events``.  The graph and its CSR are resident on the device.  Printed per size: the end-to-end median of --repeats runs
(host clock around a device synchronise) of ``color_refinement`` alone and of ``WeisfeilerLeman_test`` of the graph against a relabelled
copy of itself (integer IDs; the result is True), the rounds and verify passes, and — from one extra run that drains the stream around every
stage, so its total is larger than the untimed median — the time per round split into the key sort, the grouping (unique rows) and the new
kernels.  The host comparison is the reference's loop restated on pre-fetched successor lists (the fetching is not timed), run once and
given up after --host-limit seconds.  No threshold is attached to any time.
"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _dispatch  # noqa: E402
from pathpyg_amd.algorithms import weisfeiler_leman  # noqa: E402

DEV = "cuda:0"


def aggregated_graph(nodes: int, events: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    ei = (torch.rand((2, events), generator=g, dtype=torch.float64).pow(3) * nodes).long().clamp_(max=nodes - 1)
    t = torch.randint(0, events, (events,), generator=g)
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=nodes))
    return tg.to_static_graph()


def timed(fn, repeats: int):
    out, times = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def host_loop(succ: list, walk: list, limit: float):
    """The reference's rounds on successor lists by node index, without features; ``None`` when ``limit`` seconds did not suffice."""
    t0 = time.perf_counter()
    current = ["0"] * len(succ)
    numbers: dict = {}
    rounds = 0
    while True:
        refined = [None] * len(succ)
        for v in walk:
            around = [current[w] for w in succ[v]]
            around.sort()
            refined[v] = numbers.setdefault(str(current[v]) + str(around), len(numbers) + 1)
        rounds += 1
        if time.perf_counter() - t0 > limit:
            return None, rounds, time.perf_counter() - t0
        if len(set(current)) == len(set(refined)):
            return current, rounds, time.perf_counter() - t0
        current = refined


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000:50000,100000:1000000,1000000:10000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-limit", type=float, default=60.0)
    ap.add_argument("--out", default="profiles/wl.txt")
    args = ap.parse_args()
    alg = pp.algorithms
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        def row(name, ts):
            say(f"  {name:<44s}: median {statistics.median(ts):10.2f}   min {min(ts):10.2f}   max {max(ts):10.2f}   all {[round(x, 2) for x in ts]}")

        say(f"# tools/bench_wl.py: colour refinement / Weisfeiler-Leman test of an aggregated static graph; "
            f"{torch.cuda.get_device_name(0)}; --sizes {args.sizes} --repeats {args.repeats}; times in ms, end to end")
        alg.color_refinement(aggregated_graph(50, 300, seed=1))         # first launches load the code objects: not part of any number below
        for size in args.sizes.split(","):
            nodes, events = (int(x) for x in size.split(":"))
            g1 = aggregated_graph(nodes, events)
            n, m = g1.n, g1.data.edge_index.size(1)
            g1.mapping = pp.IndexMap(np.arange(n))
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
            g2 = pp.Graph(pp.Data(edge_index=perm[g1.data.edge_index], num_nodes=n), mapping=pp.IndexMap(np.arange(n, 2 * n)))
            g1.row_ptr, g2.row_ptr                                      # the CSRs are built once per graph, outside the timed calls
            deg = g1.row_ptr[1:] - g1.row_ptr[:-1]
            say(f"== n = {n} nodes, m = {m} stored edges (from {events} events), largest out-degree {int(deg.max())}, "
                f"{int((deg >= 1024).sum())} rows of 1024 entries or more")
            (colours, counts, passes), ts = timed(lambda: alg.color_refinement(g1, with_stats=True), args.repeats)
            row("color_refinement, one graph", ts)
            say(f"  {len(counts) - 1} rounds, classes per round {counts}, verify passes per round {passes[1:]}")
            _, stats = _dispatch.graph_color_refinement(g1, timed=True)
            per_round = [1e3 * s / max(len(stats.counts) - 1, 1) for s in stats.seconds]
            say(f"  drained run, per round: key sort {per_round[0]:.3f} ms, grouping (unique rows) {per_round[2]:.3f} ms, "
                f"new kernels (signature, election, verify, numbering) {per_round[1]:.3f} ms")
            (same, fp1, fp2), ts = timed(lambda: alg.WeisfeilerLeman_test(g1, g2), args.repeats)
            row("WeisfeilerLeman_test, graph vs relabelled copy", ts)
            stats = weisfeiler_leman.last_stats
            say(f"  result {same}; {len(stats.counts) - 1} rounds on the union of {2 * n} nodes, classes per round {stats.counts}, "
                f"verify passes per round {stats.passes[1:]}")
            ptr1, col1 = g1.row_ptr.cpu().tolist(), g1.col.cpu().tolist()
            ptr2, col2 = g2.row_ptr.cpu().tolist(), g2.col.cpu().tolist()
            succ = [col1[ptr1[v]:ptr1[v + 1]] for v in range(n)] + [[w + n for w in col2[ptr2[v]:ptr2[v + 1]]] for v in range(n)]
            want, rounds, seconds = host_loop(succ, list(range(2 * n)), args.host_limit)
            if want is None:
                say(f"  reference loop restated, host, successor lists pre-fetched: given up after {rounds} rounds and {seconds:.1f} s "
                    f"(--host-limit {args.host_limit:.0f} s)")
            else:
                say(f"  reference loop restated, host, successor lists pre-fetched: {seconds * 1e3:10.2f} ms (one run, {rounds} rounds; "
                    f"same fingerprints: {want == fp1 + fp2})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
