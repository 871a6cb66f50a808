#!/usr/bin/env python3
"""RollingTimeWindow on the headline stream of bench.py (10^7 events, 5 * 10^5 nodes, timestamps below 10^7, i.i.d. uniform): the native
pass (csrc/pp_rolling.hip) against the only route there was before it — one ``TemporalGraph.to_static_graph(weighted=True, time_window=w)``
per window — over the SAME windows, in one process, alternating, at 100 and 1000 windows, disjoint (step = size) and overlapping
(step = size / 4).

    python tools/bench_rolling.py [--out profiles/rolling.txt]                      # end-to-end times (host clock around a device synchronise)
    rocprofv3 --kernel-trace --stats -d DIR -o x -- python tools/bench_rolling.py --trace --windows 1000 --overlap 1
    python tools/bench_rolling.py --kernels DB --windows 1000 --overlap 1 [--out ...] # kernel times of that run, bytes over time against HBM

Every run of the two routes is checked to give the same graphs (edge counts, weights sums and node counts of every window; all tensors of
a sample).  The byte counts are the formula of DESIGN.md ("Rolling time windows"), from shapes alone.
"""
import argparse
import json
import sqlite3
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _hip  # noqa: E402
from pathpyg_amd.algorithms import rolling_time_window as rtw  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12             # bytes / s, MI355X specification (about 6.3e12 is what a copy kernel reaches)
ROLLING_KERNELS = ("k_roll_", "k_digit_hist", "k_scan_digit_rows", "k_scatter", "k_tile_sums", "k_scan_tile_sums", "k_scan_tiles")


def stream(events: int, nodes: int, span: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, nodes, (2, events), generator=g)
    t = torch.randint(0, span, (events,), generator=g)
    return pp.TemporalGraph(pp.Data(edge_index=ei.to(DEV), time=t.to(DEV), num_nodes=nodes))


def window_args(span: int, windows: int, overlap: int):
    step = -(-span // windows)
    return step * overlap, step


def algorithm_bytes(m: int, nodes: int, windows: int, total: int) -> dict:
    """HBM bytes the pass needs, by stage ("Rolling time windows"): K key bytes, P1 / P2 radix passes of the pair and window sorts."""
    K = torch.empty(0, dtype=_hip.rolling_key_dtype(nodes)).element_size()
    p1 = -(-(2 * max((max(nodes, 2) - 1).bit_length(), 1)) // 8)
    p2 = -(-max((windows - 1).bit_length(), 1) // 8) if windows > 1 else 0
    group = m * (16 + 8 + K) + m * (3 * K + 4 + (p1 - 1) * (3 * K + 8))
    count = m * (K + 4 + 4)
    fill = m * 12 + m * (K + 8) + total * 8
    wsort = total * p2 * 20
    emit = total * (8 + K + 4 + 20)
    return {"group": group, "count": count, "scan+fill": fill, "window sort": wsort, "emit": emit, "all": group + count + fill + wsort + emit}


def run_native(g, size, step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graphs = list(pp.algorithms.RollingTimeWindow(g, size, step))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, graphs


def run_per_window(g, size, step):
    rtw.NATIVE = False
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graphs = list(pp.algorithms.RollingTimeWindow(g, size, step))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, graphs
    finally:
        rtw.NATIVE = True


def summary(graphs):
    return [(s.data.edge_index.size(1), s.n) for s in graphs]


def same(a, b) -> bool:
    if summary(a) != summary(b):
        return False
    picks = sorted({0, len(a) // 3, len(a) // 2, len(a) - 1})
    return all(torch.equal(a[i].data.edge_index, b[i].data.edge_index) and torch.equal(a[i].data.edge_weight, b[i].data.edge_weight) for i in picks)


def timings(args, say):
    g = stream(args.events, args.nodes, args.span)
    warm = stream(20_000, 100, 1000, seed=1)                      # first launches load the code objects: not part of any number below
    run_native(warm, 10, 10), run_per_window(warm, 10, 10), run_native(warm, 40, 10)
    rows = []
    for overlap in (1, 4):
        for windows in (100, 1000):
            size, step = window_args(args.span, windows, overlap)
            times = {"native": [], "per window": []}
            for _ in range(args.repeats):
                ms, a = run_native(g, size, step)
                times["native"].append(ms)
                ms, b = run_per_window(g, size, step)
                times["per window"].append(ms)
                assert same(a, b), "the two routes returned different graphs"
                total = sum(s.data.edge_index.size(1) for s in a)
                n_windows = len(a)
                del a, b
            say(f"== {n_windows} windows of {size} time units, step {step} ({'disjoint' if overlap == 1 else 'each event in %d windows' % overlap}); "
                f"{args.events} events, {total} edges in all windows")
            for name, ts in times.items():
                say(f"  {name:<11s}: median {statistics.median(ts):10.2f} ms   min {min(ts):10.2f}   max {max(ts):10.2f}   all {[round(x, 2) for x in ts]}")
            need = algorithm_bytes(args.events, args.nodes, n_windows, total)
            say(f"  bytes the native pass needs (DESIGN formula): {need['all'] / 1e9:.3f} GB = " + ", ".join(f"{k} {v / 1e9:.3f}" for k, v in need.items() if k != "all"))
            rows.append({"windows": n_windows, "size": size, "step": step, "edges": total, "native_ms": round(statistics.median(times["native"]), 2),
                         "per_window_ms": round(statistics.median(times["per window"]), 2), "native_all_ms": [round(x, 2) for x in times["native"]],
                         "per_window_all_ms": [round(x, 2) for x in times["per window"]], "algorithm_bytes": need["all"], "same_graphs": True})
    for overlap in (1, 4):
        sel = [r for r in rows if (r["size"] == r["step"]) == (overlap == 1)]
        say(f"  step = size / {overlap}: native {sel[0]['native_ms']} ms at {sel[0]['windows']} windows -> {sel[1]['native_ms']} ms at {sel[1]['windows']} "
            f"(x{sel[1]['native_ms'] / sel[0]['native_ms']:.2f} for x{sel[1]['windows'] / sel[0]['windows']:.1f} windows); per window "
            f"{sel[0]['per_window_ms']} -> {sel[1]['per_window_ms']} ms (x{sel[1]['per_window_ms'] / sel[0]['per_window_ms']:.2f})")
    for r in rows:
        say(json.dumps(r))


def trace_target(args):
    g = stream(args.events, args.nodes, args.span)
    size, step = window_args(args.span, args.windows, args.overlap)
    for _ in range(args.repeats):
        batch = pp.algorithms.rolling_static_graphs(g, size, step)
        torch.cuda.synchronize()
    print(json.dumps({"windows": len(batch), "edges": int(batch.win_ptr_host[-1]), "repeats": args.repeats}))


def kernel_table(args, say):
    db = sqlite3.connect(args.kernels)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = db.execute(f"select {name_col}, count(*), sum(end - start), min(end - start), max(end - start) from kernels group by {name_col} "
                      "order by 3 desc").fetchall()
    rows = [r for r in rows if any(k in r[0] for k in ROLLING_KERNELS)]
    size, step = window_args(args.span, args.windows, args.overlap)
    say(f"== kernels of {args.repeats} x rolling_static_graphs, {args.windows} windows of {size}, step {step} (rocprofv3 --kernel-trace --stats, a run of its own; "
        f"the stream's own time sort shares the sort and scan kernels and is in these sums)")
    total_ns = sum(r[2] for r in rows)
    for name, calls, ns, least, most in rows:
        say(f"  {(name if len(name) <= 70 else name[:67] + '...'):<72s} {calls:>4d} calls {ns / 1e6:>9.3f} ms   min {least / 1e3:>8.1f} us   max {most / 1e3:>8.1f} us")
    per_pass_ms = total_ns / 1e6 / args.repeats
    need = algorithm_bytes(args.events, args.nodes, args.windows, args.edges)["all"] if args.edges else None
    say(f"  kernel time per pass: {per_pass_ms:.3f} ms")
    if need:
        rate = need / (per_pass_ms * 1e-3)
        say(f"  bytes needed {need / 1e9:.3f} GB / kernel time = {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak "
            f"(bound: bandwidth; least time {need / HBM_PEAK * 1e3:.3f} ms)")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--nodes", type=int, default=500_000)
    ap.add_argument("--span", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="profiles/rolling.txt")
    ap.add_argument("--trace", action="store_true", help="only run the native pass --repeats times (the program to put behind rocprofv3)")
    ap.add_argument("--kernels", default="", help="rocpd database of a --trace run: append its kernel table")
    ap.add_argument("--windows", type=int, default=1000)
    ap.add_argument("--overlap", type=int, default=1)
    ap.add_argument("--edges", type=int, default=0, help="--kernels: edges in all windows, as the --trace run printed them")
    args = ap.parse_args()
    if args.trace:
        trace_target(args)
        return 0
    with open(args.out, "a" if args.kernels else "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        if args.kernels:
            kernel_table(args, say)
        else:
            say(f"# tools/bench_rolling.py: RollingTimeWindow, native pass against the per-window loop; {torch.cuda.get_device_name(0)}; "
                f"--events {args.events} --nodes {args.nodes} --span {args.span} --repeats {args.repeats}")
            timings(args, say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
