#!/usr/bin/env python3
"""Static shortest paths and centralities (csrc/pp_graph_paths.hip) on the aggregated static graph of a seeded temporal stream whose node
choice is skewed (node = floor(nodes * u^3), u uniform: a few hubs far above one wave, most nodes with a handful of edges).

    python tools/bench_static_paths.py [--out profiles/static_paths.txt] [--sizes 1000:10000,5000:50000,20000:200000]

Each size is ``nodes:events``.  Printed per size: the end-to-end time (host clock around a device synchronise, graph resident on the device,
results back on the host as the public functions return them) of ``shortest_paths_dijkstra`` (up to --dense-limit nodes: the result is dense
n x n), ``diameter``, ``avg_path_length``, ``closeness_centrality`` and ``betweenness_centrality``.  Where scipy and networkx import, the
routes the reference takes are timed on the host for comparison and labelled as such: scipy's ``dijkstra(unweighted=True)``,
``networkx.closeness_centrality`` on a DiGraph copy, and — up to --python-limit nodes — the reference's betweenness loop restated here
(per-source Python lists and dicts over successor lists); the results of the two sides are compared.  No threshold is attached to any time.
"""
import argparse
import statistics
import sys
import time
from collections import defaultdict

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402

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


def python_betweenness(successors, n):
    """The reference's route restated: Brandes per source over successor lists with Python containers, ``bw[w] += delta[w]`` once per
    predecessor entry."""
    bw = defaultdict(float)
    for s in range(n):
        order, preds = [], defaultdict(list)
        sigma, dist = defaultdict(int), {s: 0}
        sigma[s] = 1
        queue, head = [s], 0
        while head < len(queue):
            v = queue[head]
            head += 1
            order.append(v)
            for w in successors[v]:
                if w not in dist:
                    dist[w] = dist[v] + 1
                    queue.append(w)
                if dist[w] == dist[v] + 1:
                    sigma[w] += sigma[v]
                    preds[w].append(v)
        delta = defaultdict(float)
        for w in reversed(order):
            for v in preds[w]:
                delta[v] += sigma[v] / sigma[w] * (1 + delta[w])
                bw[w] += delta[w]
    return bw


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000:10000,5000:50000,20000:200000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dense-limit", type=int, default=5000)
    ap.add_argument("--python-limit", type=int, default=1000)
    ap.add_argument("--out", default="profiles/static_paths.txt")
    args = ap.parse_args()
    try:
        import networkx as nx
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        nx = dijkstra = None
    alg = pp.algorithms
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"# tools/bench_static_paths.py: static shortest paths / closeness / betweenness on an aggregated static graph; "
            f"{torch.cuda.get_device_name(0)}; --sizes {args.sizes} --repeats {args.repeats}; times in ms, end to end")
        warm = aggregated_graph(50, 300, seed=1)                   # first launches load the code objects: not part of any number below
        alg.shortest_paths.shortest_paths_dijkstra(warm), alg.diameter(warm), alg.closeness_centrality(warm), alg.betweenness_centrality(warm)
        for size in args.sizes.split(","):
            nodes, events = (int(x) for x in size.split(":"))
            g = aggregated_graph(nodes, events)
            g.row_ptr                                                # the CSR is built once per graph, outside the timed calls
            n, m = g.n, g.data.edge_index.size(1)
            deg = (g.row_ptr[1:] - g.row_ptr[:-1])
            say(f"== n = {n} nodes, m = {m} stored edges (from {events} events), largest out-degree {int(deg.max())}, "
                f"{int((deg >= 64).sum())} rows of 64 entries or more")
            results = {}
            calls = [("diameter", lambda: alg.diameter(g)), ("avg_path_length", lambda: alg.avg_path_length(g)),
                     ("closeness_centrality", lambda: alg.closeness_centrality(g)), ("betweenness_centrality", lambda: alg.betweenness_centrality(g))]
            if n <= args.dense_limit:
                calls.insert(0, ("shortest_paths_dijkstra", lambda: alg.shortest_paths.shortest_paths_dijkstra(g)))
            for name, fn in calls:
                results[name], ts = timed(fn, args.repeats)
                say(f"  {name:<26s}: median {statistics.median(ts):10.2f}   min {min(ts):10.2f}   max {max(ts):10.2f}   all {[round(x, 2) for x in ts]}")
            say(f"  diameter {results['diameter']}, avg_path_length {results['avg_path_length']}, "
                f"{len(results['betweenness_centrality'])} betweenness keys")
            if nx is None:
                say("  reference routes: scipy / networkx do not import here")
                continue
            adj = g.sparse_adj_matrix()
            t0 = time.perf_counter()
            dist = dijkstra(adj, directed=True, return_predecessors=False, unweighted=True) if n <= args.dense_limit else None
            t_scipy = (time.perf_counter() - t0) * 1e3
            if dist is not None:
                same = np.array_equal(dist, results["shortest_paths_dijkstra"][0]) and float(np.max(dist)) == results["diameter"]
                say(f"  reference route, host: scipy dijkstra(unweighted=True) {t_scipy:10.2f} ms (one run; same distances and diameter: {same})")
            ei = g.data.edge_index.cpu()
            t0 = time.perf_counter()
            nxg = nx.DiGraph()
            nxg.add_nodes_from(range(n))
            nxg.add_edges_from(ei.T.tolist())
            t_copy = (time.perf_counter() - t0) * 1e3
            if n <= args.dense_limit:
                t0 = time.perf_counter()
                want = nx.closeness_centrality(nxg)
                t_nx = (time.perf_counter() - t0) * 1e3
                same = list(results["closeness_centrality"].values()) == [want[v] for v in range(n)]
                say(f"  reference route, host: networkx closeness_centrality {t_nx:10.2f} ms + {t_copy:.2f} ms graph copy (one run; same values bit for bit: {same})")
            if n <= args.python_limit:
                row_ptr, col = g.row_ptr.cpu().tolist(), g.col.cpu().tolist()
                successors = [col[row_ptr[v]:row_ptr[v + 1]] for v in range(n)]
                t0 = time.perf_counter()
                want = python_betweenness(successors, n)
                t_py = (time.perf_counter() - t0) * 1e3
                got = results["betweenness_centrality"]
                worst = max((abs(got[v] - want[v]) / max(abs(want[v]), 1.0) for v in want), default=0.0)
                say(f"  reference route, host: Python Brandes loop (restated) {t_py:10.2f} ms (one run; same keys: {set(got) == set(want)}, "
                    f"largest relative difference {worst:.2e})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
