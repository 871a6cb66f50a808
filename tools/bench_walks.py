#!/usr/bin/env python3
"""Time pathpyg_amd.processes.RandomWalk (csrc/pp_walks.hip) on the device and write profiles/walks.txt.

    python tools/bench_walks.py [--walks 1000000] [--steps 10,100] [--repeats 3] [--out profiles/walks.txt] [--graphs gnp5,gnp6,hub,layer2]

Graphs: G(n,p) with 10^5 and 10^6 nodes and mean degree 10 (``erdos_renyi_gnp``, undirected: both directions stored); the aggregated static
graph of the seeded hub stream tools/bench_static_paths.py uses (node = floor(nodes * u^3): a few rows far above a wave), weighted by its
edge counts; layer 2 of the model of bench.py's headline stream (10^7 events, 5 * 10^5 nodes, timestamps below 10^7, delta 10^6), weighted.
Per graph and step count, the median of ``--repeats`` runs after one warm-up, the stream drained around every stage: the transition table
(once per RandomWalk), the walk kernel, the pack into PathData tensors, and the public call ``run(...).to_path_data()`` on a fresh
RandomWalk (table included).  Steps per second = edges walked / walk kernel time.  The comparison line is the same sampling restated in
numpy, vectorised per step over all walks (its own random stream: the cost is what is compared), run on the host once.  There is no
acceptance threshold on any of these times.
"""
from __future__ import annotations

import argparse
import datetime
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _hip  # noqa: E402
from pathpyg_amd.algorithms import generative_models as gm  # noqa: E402

DEV = "cuda:0"


def timed(fn, repeats):
    fn()                                                                # warm-up: allocator, code objects
    out, times = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times)


def hub_graph(nodes=1_000_000, events=10_000_000, seed=0):
    g = torch.Generator().manual_seed(seed)
    ei = (torch.rand((2, events), generator=g, dtype=torch.float64).pow(3) * nodes).long().clamp_(max=nodes - 1)
    t = torch.randint(0, events, (events,), generator=g)
    return pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=nodes)).to_static_graph(weighted=True)


def headline_layer2(events=10_000_000, nodes=500_000, span=10_000_000, delta=1_000_000, seed=0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, nodes, (2, events), generator=g)
    t = torch.randint(0, span, (events,), generator=g)
    tg = pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=nodes))
    layer = pp.MultiOrderModel.from_temporal_graph(tg, delta=delta, max_order=2).layers[2]
    layer.data.edge_index, layer.data.edge_weight, layer.data.node_sequence        # (deferred tensors: made here, not inside a timed stage)
    return layer


def numpy_walks(row_ptr, col, weight, walks, steps, seed=1):
    """The same sampling on the host, vectorised per step: cumulative weights once, then per step one searchsorted over all walks."""
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    w = np.ones(col.size) if weight is None else weight.astype(np.float64)
    glob = np.cumsum(w)                                                 # (global running sums: the host's cheap stand-in for row-local ones)
    base = np.concatenate(([0.0], glob))[row_ptr[:-1]]
    total = np.concatenate(([0.0], glob))[row_ptr[1:]] - base
    table = time.perf_counter() - t0
    t0 = time.perf_counter()
    start_cum = np.cumsum(total)
    v = np.searchsorted(start_cum, rng.random(walks) * start_cum[-1], side="right")
    alive = np.ones(walks, dtype=bool)
    edges = 0
    for _ in range(steps):
        alive &= total[v] > 0
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        at = v[idx]
        j = np.searchsorted(glob, base[at] + rng.random(idx.size) * total[at], side="right")
        v[idx] = col[np.minimum(j, row_ptr[at + 1] - 1)]
        edges += idx.size
    return table, time.perf_counter() - t0, edges


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--walks", type=int, default=1_000_000)
    ap.add_argument("--steps", default="10,100")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--graphs", default="gnp5,gnp6,hub,layer2")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy comparison")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "walks.txt"))
    args = ap.parse_args()
    makers = {
        "gnp5": ("G(n,p) n=1e5 deg 10", None, lambda: gm.erdos_renyi_gnp(100_000, 10 / 99_999, seed=7, device=DEV)),
        "gnp6": ("G(n,p) n=1e6 deg 10", None, lambda: gm.erdos_renyi_gnp(1_000_000, 10 / 999_999, seed=7, device=DEV)),
        "hub": ("hub stream, aggregated", "edge_weight", hub_graph),
        "layer2": ("headline stream, layer 2", "edge_weight", headline_layer2),
    }
    W = args.walks
    lines = [f"# tools/bench_walks.py, {datetime.date.today().isoformat()}: {W} walks, start \"weighted\", medians of {args.repeats} after one warm-up, "
             f"milliseconds; device: {torch.cuda.get_device_name(0)}",
             "# graph                         n          m  steps | table ms | walk ms | pack ms | public ms | edges walked | steps/s (walk kernel) | "
             "numpy: table ms, walk ms, steps/s"]
    print("\n".join(lines), flush=True)
    for key in args.graphs.split(","):
        name, weight, make = makers[key]
        graph = make()
        graph.row_ptr                                                   # (the CSR pointers belong to the Graph, not to the sampler)
        n, m = graph.n, int(graph.data.edge_index.size(1))
        _, table_s = timed(lambda: pp.processes.RandomWalk(graph, weight=weight).table(), args.repeats)
        rw = pp.processes.RandomWalk(graph, weight=weight)
        rw.run(num_walks=16, steps=1, seed=1)                           # tables built
        for steps in [int(x) for x in args.steps.split(",")]:
            batch, walk_s = timed(lambda: rw.run(num_walks=W, steps=steps, seed=7), args.repeats)
            edges = int(batch.lengths.sum())
            _, pack_s = timed(lambda: _hip.walk_pack(batch.steps_major, batch._lengths32, batch._node_sequence, n), args.repeats)
            _, public_s = timed(lambda: pp.processes.RandomWalk(graph, weight=weight).run(num_walks=W, steps=steps, seed=7).to_path_data(),
                                args.repeats)
            host = "-"
            if not args.no_host:
                hw = None if weight is None else graph.data[weight].cpu().numpy()
                ht, hs, he = numpy_walks(graph.row_ptr.cpu().numpy(), graph.col.cpu().numpy(), hw, W, steps)
                host = f"{ht * 1e3:.1f}, {hs * 1e3:.1f}, {he / hs:.3e}"
            line = (f"{name:<26} {n:>9} {m:>10} {steps:>6} | {table_s * 1e3:.3f} | {walk_s * 1e3:.3f} | {pack_s * 1e3:.3f} | {public_s * 1e3:.3f} | "
                    f"{edges} | {edges / walk_s:.3e} | {host}")
            print(line, flush=True)
            lines.append(line)
            del batch
        del rw, graph
        torch.cuda.empty_cache()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
