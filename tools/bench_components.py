#!/usr/bin/env python3
"""Connected components and the largest component (csrc/pp_graph_components.hip) on the aggregated static graph of the seeded temporal stream
tools/bench_static_paths.py uses (node = floor(nodes * u^3), u uniform: a few hubs far above one wave, most nodes with a handful of edges).

    python tools/bench_components.py [--out profiles/components.txt] [--sizes 5000:50000,100000:1000000,1000000:10000000]

Each size is ``nodes:events``.  Printed per size: the end-to-end median of --repeats runs (host clock around a device synchronise, graph and
its CSR / CSC resident on the device, results as the public functions return them: labels on the host, the sub-graph on the device) of
``connected_components`` weak and strong and of ``largest_connected_component`` weak, and the kernel's counters (rounds, trim / colour /
backward sweeps).  Where scipy imports, the route the reference takes is timed on the host and labelled as such:
``graph.sparse_adj_matrix()`` + ``scipy.sparse.csgraph.connected_components``, and — up to --python-limit stored edges — its per-edge Python
loop over ``graph.edges`` restated here; the results of the two sides are compared.  Last, a star whose hub has the largest or the smallest
index: every edge of the first meets the others on the hub's word.  No threshold is attached to any time.
"""
import argparse
import statistics
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _dispatch  # noqa: E402

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


def by_first_appearance(labels: np.ndarray) -> np.ndarray:
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


def python_lcc(graph, labels):
    """The reference's route restated: Counter over the labels, then a loop over graph.edges with two mapping lookups per edge."""
    x, _ = Counter(labels.tolist()).most_common(1)[0]
    kept = []
    for v, w in graph.edges:
        if labels[graph.mapping.to_idx(v)] == x and labels[graph.mapping.to_idx(w)] == x:
            kept.append((v, w))
    return kept


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000:50000,100000:1000000,1000000:10000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--python-limit", type=int, default=1_000_000)
    ap.add_argument("--out", default="profiles/components.txt")
    args = ap.parse_args()
    try:
        from scipy.sparse.csgraph import connected_components as scipy_cc
    except ImportError:
        scipy_cc = None
    alg = pp.algorithms
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        def row(name, ts):
            say(f"  {name:<38s}: median {statistics.median(ts):10.2f}   min {min(ts):10.2f}   max {max(ts):10.2f}   all {[round(x, 2) for x in ts]}")

        say(f"# tools/bench_components.py: connected components / largest component of an aggregated static graph; "
            f"{torch.cuda.get_device_name(0)}; --sizes {args.sizes} --repeats {args.repeats}; times in ms, end to end")
        warm = aggregated_graph(50, 300, seed=1)                    # first launches load the code objects: not part of any number below
        alg.connected_components(warm), alg.connected_components(warm, "strong"), alg.largest_connected_component(warm)
        for size in args.sizes.split(","):
            nodes, events = (int(x) for x in size.split(":"))
            g = aggregated_graph(nodes, events)
            g.row_ptr, g.col_ptr                                    # CSR and CSC are built once per graph, outside the timed calls
            n, m = g.n, g.data.edge_index.size(1)
            deg = g.row_ptr[1:] - g.row_ptr[:-1]
            say(f"== n = {n} nodes, m = {m} stored edges (from {events} events), largest out-degree {int(deg.max())}, "
                f"{int((deg >= 64).sum())} rows of 64 entries or more")
            (cw, weak), ts = timed(lambda: alg.connected_components(g), args.repeats)
            row("connected_components weak", ts)
            (cs, strong), ts = timed(lambda: alg.connected_components(g, "strong"), args.repeats)
            row("connected_components strong", ts)
            lcc, ts = timed(lambda: alg.largest_connected_component(g), args.repeats)
            row("largest_connected_component weak", ts)
            _, ts = timed(lambda: _dispatch.graph_components(g, False), args.repeats)
            row("  labels and sizes left on the device, weak", ts)
            stats = _dispatch.graph_components(g, True, with_stats=True)[3]
            say(f"  weak: {cw} components, largest {np.bincount(weak).max()}; strong: {cs} components, largest {np.bincount(strong).max()}; "
                f"largest weak component as a graph: n = {lcc.n}, {lcc.data.edge_index.size(1)} stored edges")
            say(f"  strong counters: {stats[0]} rounds, {stats[1]} trim sweeps, {stats[2]} colour sweeps, {stats[3]} backward sweeps")
            if scipy_cc is None:
                say("  reference route: scipy does not import here")
                continue
            for connection, mine in (("weak", weak), ("strong", strong)):
                t0 = time.perf_counter()
                count, want = scipy_cc(g.sparse_adj_matrix(), directed=True, connection=connection, return_labels=True)
                t_ref = (time.perf_counter() - t0) * 1e3
                same = count == (cw if connection == "weak" else cs) and np.array_equal(by_first_appearance(want), mine)
                say(f"  reference route, host: sparse_adj_matrix() + scipy connected_components {connection:<6s} {t_ref:10.2f} ms "
                    f"(one run; same count and partition: {same})")
            if m <= args.python_limit:
                t0 = time.perf_counter()
                kept = python_lcc(g, weak)
                t_loop = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                want = pp.Graph.from_edge_list(kept, device=g.device)
                t_build = (time.perf_counter() - t0) * 1e3
                same = want.n == lcc.n and torch.equal(want.data.edge_index, lcc.data.edge_index) and \
                    np.array_equal(np.asarray(want.mapping.node_ids), np.asarray(lcc.mapping.node_ids))
                say(f"  reference route, host: per-edge Python loop over graph.edges (restated) {t_loop:10.2f} ms + from_edge_list {t_build:.2f} ms, "
                    f"after the labels (one run; same graph: {same})")
            else:
                say(f"  reference route, host: per-edge Python loop not run above --python-limit {args.python_limit} stored edges")
        leaves = 1_000_000
        say(f"== star of {leaves} leaves, edges leaf -> hub: all edges share the hub")
        for name, hub, first in (("hub has the largest index", leaves, 0), ("hub has index 0", 0, 1)):
            ei = torch.stack((torch.arange(first, first + leaves), torch.full((leaves,), hub))).to(DEV)
            star = pp.Graph(pp.Data(edge_index=ei, num_nodes=leaves + 1))
            (count, _, _), ts = timed(lambda: _dispatch.graph_components(star, False), args.repeats + 1)
            row(f"weak, on the device, {name}", ts[1:])
            assert int(count.item()) == 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
