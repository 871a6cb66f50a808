"""read_csv_temporal_graph(device="cuda") on an integer `v,w,t` file: the native ingest (csrc/pp_ingest.hip) against the pandas path
(io.pandas.NATIVE_CSV = False, what the function did before), on the SAME file, in one process, alternating.

Two files under a temporary directory: the headline stream of bench.py (10^7 events, 5 * 10^5 nodes, timestamps below 10^7, i.i.d. uniform)
and a 10^5-event one.  Per file: the whole call of either path (host clock around a call that ends in a device synchronise), then the
phases of either path, one line each — the native ones by the same calls io/pandas.py makes, each with a host clock (synchronised) and,
for the device phases, device events.  The two paths must return the same graph.  One JSON line per file at the end.

    python tools/probes/ingest.py [--rows 10000000 100000] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _hip  # noqa: E402
from pathpyg_amd.io import pandas as ppio  # noqa: E402

DEV = "cuda:0"


def write_stream(path: str, rows: int, nodes: int, span: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    frame = pd.DataFrame({"v": rng.integers(0, nodes, rows), "w": rng.integers(0, nodes, rows), "t": rng.integers(0, span, rows)})
    frame.to_csv(path, index=False)


class Phases:
    """name -> list of (wall ms, device ms or None)"""

    def __init__(self):
        self.rows = {}

    def run(self, name, step, device=True):
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        out = step()
        stop.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        self.rows.setdefault(name, []).append((wall, start.elapsed_time(stop) if device else None))
        return out

    def report(self, title):
        print(title)
        total = 0.0
        for name, samples in self.rows.items():
            wall = statistics.median(s[0] for s in samples)
            total += wall
            dev = "" if samples[0][1] is None else f"   device events {statistics.median(s[1] for s in samples):10.3f} ms"
            print(f"    {name:<34s} wall {wall:10.3f} ms{dev}   (min {min(s[0] for s in samples):.3f}, max {max(s[0] for s in samples):.3f}, n={len(samples)})")
        print(f"    {'sum of the phases':<34s} wall {total:10.3f} ms")
        return {name: round(statistics.median(s[0] for s in samples), 3) for name, samples in self.rows.items()}


def native_phases(path: str, ph: Phases):
    """The steps of io.pandas._read_csv_temporal_native (header=True, sep=',', time_rescale=1, multiedges=False), timed one by one."""
    raw = ph.run("file read (np.fromfile)", lambda: np.fromfile(path, dtype=np.uint8), device=False)
    start = ppio._header_length(raw[:8].tobytes(), ",")
    chunks = ph.run("chunk cut (host)", lambda: ppio._cut_chunks(raw, ppio.CHUNK_BYTES, start), device=False)
    parts = []
    for lo, hi in chunks:
        chunk = ph.run("copy to the device", lambda: torch.from_numpy(raw[lo:hi]).to(DEV))
        ws = _hip.ingest_workspace(hi - lo, chunk.device)
        line_start = ph.run("line index", lambda: _hip.ingest_index(chunk, ord(","), ws))
        cols = ph.run("parse", lambda: _hip.ingest_parse(chunk, ord(","), line_start, ws))
        n_lines, status, _ = ph.run("status read-back", lambda: _hip.ingest_result(ws), device=False)
        assert status == 0, status
        parts.append(ph.run("trim to the line count", lambda: cols[:, :n_lines].clone()))
        del chunk, ws, line_start, cols
    cols = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    v, w, t = cols[0], cols[1], cols[2]

    def dedupe():
        keep = ppio._first_occurrences(torch.stack([v, w, t], dim=1))
        return (v, w, t) if keep is None else (v[keep], w[keep], t[keep])

    v, w, t = ph.run("dedupe (first occurrences)", dedupe)

    def ids_step():
        ids, inverse = _hip.unique_rows(torch.stack([v, w], dim=1).reshape(-1, 1))
        return ids.view(-1).cpu().numpy(), inverse.view(-1, 2).t().contiguous()

    ids, edge_index = ph.run("ids (unique + inverse, ids to host)", ids_step)
    return ph.run("IndexMap + TemporalGraph", lambda: pp.TemporalGraph(pp.Data(edge_index=edge_index, time=t.contiguous(), num_nodes=len(ids)),
                                                            mapping=pp.IndexMap(ids)))


def pandas_phases(path: str, ph: Phases):
    """The pandas path (io.pandas.df_to_temporal_graph) step by step."""
    df = ph.run("pandas.read_csv", lambda: pd.read_csv(path, header=0, sep=","), device=False)
    df = ph.run("drop_duplicates", lambda: df.drop_duplicates(subset=["v", "w", "t"]), device=False)
    ids, inverse = ph.run("np.unique(return_inverse)", lambda: np.unique(df[["v", "w"]].values, return_inverse=True), device=False)

    def to_device():
        edge_index = torch.from_numpy(inverse.reshape(-1, 2).T.astype(np.int64)).contiguous().to(DEV)
        return edge_index, torch.tensor(df["t"].values, device=DEV)

    edge_index, t = ph.run("tensors to the device", to_device)
    return ph.run("IndexMap + TemporalGraph", lambda: pp.TemporalGraph(pp.Data(edge_index=edge_index, time=t, num_nodes=len(ids)), mapping=pp.IndexMap(ids)))


def whole_call(path: str, native: bool) -> tuple:
    ppio.NATIVE_CSV = native
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = pp.io.read_csv_temporal_graph(path, device=DEV)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    ppio.NATIVE_CSV = True
    return ms, g


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000_000, 100_000])
    ap.add_argument("--nodes", type=int, default=500_000)
    ap.add_argument("--span", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    torch.zeros(1, device=DEV)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        warm = os.path.join(tmp, "warm.csv")                   # first launches load the code objects: not part of any number below
        write_stream(warm, 1000, 100, 1000, 1)
        whole_call(warm, True), whole_call(warm, False)
        for rows in args.rows:
            path = os.path.join(tmp, f"stream_{rows}.csv")
            t0 = time.perf_counter()
            write_stream(path, rows, args.nodes, args.span, 0)
            size = os.path.getsize(path)
            print(f"== {rows} rows, {size / 1e6:.1f} MB (written in {time.perf_counter() - t0:.1f} s)")
            times = {True: [], False: []}
            graphs = {}
            for _ in range(args.repeats):
                for native in (True, False):
                    ms, graphs[native] = whole_call(path, native)
                    times[native].append(ms)
            a, b = graphs[True], graphs[False]
            same = bool(torch.equal(a.data.edge_index, b.data.edge_index) and torch.equal(a.data.time, b.data.time)
                        and a.data.num_nodes == b.data.num_nodes and np.array_equal(a.mapping.node_ids, b.mapping.node_ids))
            assert same, "the two paths returned different graphs"
            events = int(a.data.time.numel())
            del graphs, a, b
            for native in (True, False):
                name = "native (NATIVE_CSV = True) " if native else "pandas (NATIVE_CSV = False)"
                print(f"  read_csv_temporal_graph, {name}: median {statistics.median(times[native]):10.2f} ms   all {[round(x, 2) for x in times[native]]}")
            ph_native, ph_pandas = Phases(), Phases()
            for _ in range(args.repeats):
                native_phases(path, ph_native)
                pandas_phases(path, ph_pandas)
            rep_native = ph_native.report("  phases, native path")
            rep_pandas = ph_pandas.report("  phases, pandas path")
            lines.append({"rows": rows, "file_bytes": size, "events_after_dedupe": events, "same_graph": same,
                          "native_ms": round(statistics.median(times[True]), 2), "pandas_ms": round(statistics.median(times[False]), 2),
                          "native_all_ms": [round(x, 2) for x in times[True]], "pandas_all_ms": [round(x, 2) for x in times[False]],
                          "native_phases_ms": rep_native, "pandas_phases_ms": rep_pandas})
    for line in lines:
        print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
