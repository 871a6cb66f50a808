#!/usr/bin/env python3
"""Graph statistics (csrc/pp_graph_triads.hip) on the aggregated static graph of the seeded temporal stream tools/bench_components.py uses
(node = floor(nodes * u^3), u uniform: a few hubs far above one wave, most nodes with a handful of edges).

    python tools/bench_statistics.py [--out profiles/statistics.txt] [--sizes 5000:50000,100000:1000000,1000000:10000000]

Each size is ``nodes:events``.  Printed per size: the end-to-end median of --repeats runs (host clock around a device synchronise, the graph,
its CSR and its simple successor structure resident on the device, results as the public functions return them) of ``closed_triad_counts``,
``avg_clustering_coefficient``, ``degree_assortativity`` and ``node_similarities.pairwise(..., "jaccard")`` on --pairs uniformly random
pairs; then the triad pass alone for every group width and workgroup threshold of --sweep (the numbers behind the defaults).  Where scipy
imports, the host route ``(A @ A).multiply(A).sum(1)`` on the de-duplicated adjacency matrix is timed in a child process that never opens
the device and is ended after --host-limit seconds (sizes it does not finish are reported as such), and its counts are compared with the
device's.  At the smallest size the reference's per-node loop is restated on successor lists fetched once (the reference fetches them
from the graph inside the loop, which is slower still), ended after --host-limit seconds.  No threshold is attached to any time.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _dispatch, _hip  # noqa: E402

DEV = "cuda:0"

SCIPY_CHILD = """
import sys, time
import numpy as np
from scipy.sparse import csr_matrix
ei = np.load(sys.argv[1])
n = int(sys.argv[2])
t0 = time.perf_counter()
a = csr_matrix((np.ones(ei.shape[1]), (ei[0], ei[1])), shape=(n, n))
a.data[:] = 1.0                                   # duplicates were summed: back to the set of edges
t = np.asarray((a @ a).multiply(a).sum(1)).reshape(-1).astype(np.int64)
print(time.perf_counter() - t0)
np.save(sys.argv[3], t)
"""


def aggregated_graph(nodes: int, events: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    ei = (torch.rand((2, events), generator=g, dtype=torch.float64).pow(3) * nodes).long().clamp_(max=nodes - 1)
    t = torch.randint(0, events, (events,), generator=g)
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=nodes))
    return tg.to_static_graph()


def default_width(n: int, entries: int) -> int:
    """The library's choice (include/pathpyg_amd.h): the smallest power of two no less than the mean list length, between 4 and 64."""
    mean, width = -(-entries // max(n, 1)), 4
    while width < 64 and width < mean:
        width *= 2
    return width


def timed(fn, repeats: int):
    out, times = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, times


def scipy_route(graph, limit: float):
    """``(seconds, counts)`` of the host route in a child process, ``(None, None)`` if it did not finish within ``limit`` seconds."""
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "ei.npy"), os.path.join(tmp, "t.npy")
        np.save(src, graph.data.edge_index.cpu().numpy())
        try:
            r = subprocess.run([sys.executable, "-c", SCIPY_CHILD, src, str(graph.n), dst], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            return None, None
        if r.returncode != 0:
            return None, r.stderr.strip().splitlines()[-1:] or ["failed"]
        return float(r.stdout.strip()), np.load(dst)


def python_loop(graph, limit: float):
    """The reference's closed_triads / local_clustering_coefficient loop over all nodes, restated on lists fetched once."""
    ptr, col = graph.row_ptr.cpu().tolist(), graph.col.cpu().tolist()
    succ = [col[ptr[v]:ptr[v + 1]] for v in range(graph.n)]
    t0 = time.perf_counter()
    counts = []
    for v in range(graph.n):
        edges = set()
        for x in succ[v]:
            for y in succ[x]:
                edges.add((x, y))
        mine = succ[v]
        counts.append(len({(x, y) for x, y in edges if y in mine}))
        if time.perf_counter() - t0 > limit:
            break
    return time.perf_counter() - t0, counts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000:50000,100000:1000000,1000000:10000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--sweep", default="4,8,16,32,64:256,1024,4096")
    ap.add_argument("--host-limit", type=float, default=60.0)
    ap.add_argument("--out", default="profiles/statistics.txt")
    args = ap.parse_args()
    try:
        import scipy.sparse  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    st, ns = pp.statistics, pp.statistics.node_similarities
    widths, heavies = ([int(x) for x in part.split(",")] for part in args.sweep.split(":"))
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        def row(name, ts):
            say(f"  {name:<46s}: median {statistics.median(ts):10.2f}   min {min(ts):10.2f}   max {max(ts):10.2f}   all {[round(x, 2) for x in ts]}")

        say(f"# tools/bench_statistics.py: clustering, assortativity and pair similarities of an aggregated static graph; "
            f"{torch.cuda.get_device_name(0)}; --sizes {args.sizes} --repeats {args.repeats} --pairs {args.pairs}; times in ms, end to end")
        warm = aggregated_graph(50, 300, seed=1)                    # first launches load the code objects: not part of any number below
        st.closed_triad_counts(warm), st.avg_clustering_coefficient(warm), st.degree_assortativity(warm)
        ns.pairwise(warm, torch.zeros((2, 4), dtype=torch.int64, device=DEV), "jaccard")
        first = True
        for size in args.sizes.split(","):
            nodes, events = (int(x) for x in size.split(":"))
            g = aggregated_graph(nodes, events)
            g.row_ptr                                               # the CSR is built once per graph, outside the timed calls
            _, ts = timed(lambda: g.simple_successors(), 1)
            n, m = g.n, g.data.edge_index.size(1)
            deg = g.row_ptr[1:] - g.row_ptr[:-1]
            say(f"== n = {n} nodes, m = {m} stored edges (from {events} events), largest out-degree {int(deg.max())}, "
                f"{int((deg >= 1024).sum())} rows of 1024 entries or more; simple structure (check kernel, "
                f"{'already sorted' if g._simple[3] is None else 'coalesced'}) {ts[0]:.2f} ms once")
            counts, ts = timed(lambda: st.closed_triad_counts(g), args.repeats)
            row("closed_triad_counts", ts)
            avg, ts = timed(lambda: st.avg_clustering_coefficient(g), args.repeats)
            row("avg_clustering_coefficient", ts)
            r, ts = timed(lambda: st.degree_assortativity(g), args.repeats)
            row("degree_assortativity", ts)
            gen = torch.Generator().manual_seed(7)
            pairs = torch.randint(0, n, (2, args.pairs), generator=gen).to(DEV)
            jac, ts = timed(lambda: ns.pairwise(g, pairs, "jaccard"), args.repeats)
            row(f"pairwise jaccard, {args.pairs} random pairs", ts)
            say(f"  closed triads in all: {int(counts.sum())}, most around one node {int(counts.max())}; avg clustering {avg:.6f}; "
                f"assortativity {r:.6f}; mean jaccard {float(jac.mean()):.6f}")
            if not first:                                           # (the smallest size is launch-bound: nothing to choose there)
                say("  triad pass alone (device tensor out) by group width x workgroup threshold, median of "
                    f"{args.repeats}; default: width {default_width(n, g._simple[2].numel())}, threshold 1024")
                for width in widths:
                    cells = []
                    for heavy in heavies:
                        _hip.TRIAD_GROUP, _hip.TRIAD_HEAVY_MIN = width, heavy
                        got, ts = timed(lambda: _dispatch.graph_triad_counts(g), args.repeats)
                        assert torch.equal(got, counts)
                        cells.append(f"{heavy}: {statistics.median(ts):9.2f}")
                    say(f"    width {width:2d}   " + "   ".join(cells))
                _hip.TRIAD_GROUP = _hip.TRIAD_HEAVY_MIN = None
            if have_scipy:
                seconds, want = scipy_route(g, args.host_limit)
                if seconds is None:
                    say(f"  host route, scipy (A @ A).multiply(A).sum(1): not finished within {args.host_limit:.0f} s" +
                        (f" ({want[0]})" if want else ""))
                else:
                    say(f"  host route, scipy (A @ A).multiply(A).sum(1) on the de-duplicated matrix {seconds * 1e3:10.2f} ms "
                        f"(one run, child process; same counts: {np.array_equal(want, counts.cpu().numpy())})")
            else:
                say("  host route: scipy does not import here")
            if first:
                seconds, want = python_loop(g, args.host_limit)
                same = want == counts.cpu().tolist()[:len(want)]
                say(f"  host route, the reference's per-node loop restated on lists fetched once: {len(want)} of {n} nodes in "
                    f"{seconds * 1e3:.2f} ms (one run; same counts: {same})")
            first = False
    return 0


if __name__ == "__main__":
    sys.exit(main())
