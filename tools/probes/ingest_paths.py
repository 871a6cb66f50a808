"""read_csv_path_data(device="cuda") on an integer n-gram file: the native ingest (csrc/pp_ingest.hip, the pp_ingest_tokens_* half) against
the host code (io.pandas.NATIVE_CSV = False: csv.reader, ast.literal_eval, PathData.append_walks — what the function did before), on the
SAME file, in one process, alternating.

One file per --walks value under a temporary directory: walks of 2 to 11 nodes over 5 * 10^4 integer IDs, integer weights.  Per file:
the whole call of either path (host clock around a call that ends in a device synchronise), then the phases of either path, one line
each — the native ones by the same calls io/pandas.py makes, each with a host clock (synchronised) and, for the device phases, device
events.  The two paths must return the same PathData.  One JSON line per file at the end; everything printed is also appended to --out.

    python tools/probes/ingest_paths.py [--walks 200000 2000000] [--repeats 3] [--host-repeats 3] [--out profiles/ingest_paths.txt]
"""
import argparse
import ast
import csv
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import _hip  # noqa: E402
from pathpyg_amd.io import pandas as ppio  # noqa: E402

DEV = "cuda:0"
OUT = []


def say(line: str) -> None:
    print(line, flush=True)
    OUT.append(line)


def write_walks(path: str, walks: int, ids: int, seed: int) -> int:
    rng = np.random.default_rng(seed)
    lengths = rng.integers(2, 12, walks)
    nodes = rng.integers(0, ids, int(lengths.sum())).astype(str).tolist()
    weights = rng.integers(1, 100, walks).astype(str).tolist()
    ends = np.cumsum(lengths).tolist()
    with open(path, "w") as fh:
        lo = 0
        for i, hi in enumerate(ends):
            fh.write(",".join(nodes[lo:hi]) + "," + weights[i] + "\n")
            lo = hi
    return int(lengths.sum())


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
        say(title)
        total = 0.0
        for name, samples in self.rows.items():
            wall = statistics.median(s[0] for s in samples)
            total += wall
            dev = "" if samples[0][1] is None else f"   device events {statistics.median(s[1] for s in samples):10.3f} ms"
            say(f"    {name:<38s} wall {wall:10.3f} ms{dev}   (min {min(s[0] for s in samples):.3f}, max {max(s[0] for s in samples):.3f}, n={len(samples)})")
        say(f"    {'sum of the phases':<38s} wall {total:10.3f} ms")
        return {name: round(statistics.median(s[0] for s in samples), 3) for name, samples in self.rows.items()}


def native_phases(path: str, ph: Phases):
    """The steps of io.pandas._read_csv_paths_native (weight=True, sep=','), timed one by one."""
    raw = ph.run("file read (np.fromfile)", lambda: np.fromfile(path, dtype=np.uint8), device=False)
    chunks = ph.run("chunk cut (host)", lambda: ppio._cut_chunks(raw, ppio.CHUNK_BYTES), device=False)
    parts = []
    for lo, hi in chunks:
        chunk = ph.run("copy to the device", lambda: torch.from_numpy(raw[lo:hi]).to(DEV))
        ws = _hip.ingest_tokens_workspace(hi - lo, chunk.device)
        index = ph.run("token index", lambda: _hip.ingest_tokens_index(chunk, ord(","), ws))
        nodes, lengths, weights = ph.run("parse", lambda: _hip.ingest_tokens_parse(chunk, ord(","), True, index, ws))
        n_lines, n_tokens, status, _ = ph.run("status read-back", lambda: _hip.ingest_tokens_result(ws), device=False)
        assert status == 0, status
        parts.append(ph.run("trim to the counts", lambda: (nodes[:n_tokens - n_lines].clone(), lengths[:n_lines].clone(), weights[:n_lines].clone())))
        del chunk, ws, index, nodes, lengths, weights
    nodes, lengths, weights = (parts[0] if len(parts) == 1 else tuple(torch.cat([p[k] for p in parts]) for k in range(3)))

    def ids_step():
        ids, inverse = _hip.unique_rows(nodes.view(-1, 1))
        return ids.view(-1).cpu().numpy(), inverse

    ids, inverse = ph.run("ids (unique + inverse, ids to host)", ids_step)
    node_ids, rank = ph.run("string order of the ids (host)", lambda: ppio._string_order(ids), device=False)
    node_idx = ph.run("rank to the device, gather", lambda: torch.from_numpy(rank).to(DEV)[inverse])

    def assemble():
        positions = nodes.numel()
        pos = torch.arange(positions, device=DEV)
        last = torch.zeros(positions, dtype=torch.bool, device=DEV)
        last[torch.cumsum(lengths, 0) - 1] = True
        tails = pos[~last]
        out = pp.PathData(pp.IndexMap(node_ids), torch.device(DEV))
        out._append(torch.stack((tails, tails + 1)), node_idx.unsqueeze(1), weights, lengths)
        return out

    return ph.run("IndexMap + chain + PathData", assemble)


def host_phases(path: str, ph: Phases):
    """The host code of read_csv_path_data step by step."""
    def rows_step():
        with open(path, "r") as fh:
            return [r for r in csv.reader(fh, delimiter=",") if r]

    rows = ph.run("csv.reader", rows_step, device=False)
    paths = [r[:-1] for r in rows]
    weights = ph.run("ast.literal_eval of the weights", lambda: [ast.literal_eval(r[-1]) for r in rows], device=False)
    mapping = pp.IndexMap()
    ph.run("np.unique(np.hstack(paths))", lambda: mapping.add_ids(np.unique(np.hstack(paths))), device=False)
    out = pp.PathData(mapping, DEV)
    ph.run("PathData.append_walks", lambda: out.append_walks(node_seqs=paths, weights=weights))
    return out


def whole_call(path: str, native: bool) -> tuple:
    ppio.NATIVE_CSV = native
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    paths = pp.io.read_csv_path_data(path, device=DEV)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    ppio.NATIVE_CSV = True
    return ms, paths


def same_paths(a, b) -> bool:
    return bool(all(a.data[k].dtype == b.data[k].dtype and torch.equal(a.data[k], b.data[k])
                    for k in ("edge_index", "node_sequence", "dag_weight", "dag_num_edges", "dag_num_nodes"))
                and a.data.num_nodes == b.data.num_nodes and a.mapping.node_ids.dtype == b.mapping.node_ids.dtype
                and np.array_equal(a.mapping.node_ids, b.mapping.node_ids))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks", type=int, nargs="+", default=[200_000, 2_000_000])
    ap.add_argument("--ids", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=None, help="whole calls of the host code (default: --repeats); its phases are timed once")
    ap.add_argument("--out", default="profiles/ingest_paths.txt")
    args = ap.parse_args()
    host_repeats = args.host_repeats if args.host_repeats is not None else args.repeats
    torch.zeros(1, device=DEV)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        warm = os.path.join(tmp, "warm.ngram")                 # first launches load the code objects: not part of any number below
        write_walks(warm, 1000, 100, 1)
        whole_call(warm, True), whole_call(warm, False)
        for walks in args.walks:
            path = os.path.join(tmp, f"walks_{walks}.ngram")
            t0 = time.perf_counter()
            positions = write_walks(path, walks, args.ids, 0)
            size = os.path.getsize(path)
            say(f"== {walks} walks, {positions} positions, {size / 1e6:.1f} MB (written in {time.perf_counter() - t0:.1f} s)")
            times = {True: [], False: []}
            stores = {}
            for r in range(max(args.repeats, host_repeats)):
                for native in (True, False):
                    if r < (args.repeats if native else host_repeats):
                        ms, stores[native] = whole_call(path, native)
                        times[native].append(ms)
                        print(f"  ... {'native' if native else 'host'} call {r + 1}: {ms:.2f} ms", flush=True)
            same = same_paths(stores[True], stores[False])
            assert same, "the two paths returned different walk stores"
            del stores
            native_ms, host_ms = statistics.median(times[True]), statistics.median(times[False])
            say(f"  read_csv_path_data, native (NATIVE_CSV = True) : median {native_ms:10.2f} ms   all {[round(x, 2) for x in times[True]]}")
            say(f"  read_csv_path_data, host   (NATIVE_CSV = False): median {host_ms:10.2f} ms   all {[round(x, 2) for x in times[False]]}")
            say(f"  host / native: {host_ms / native_ms:.1f}")
            ph_native, ph_host = Phases(), Phases()
            for _ in range(args.repeats):
                native_phases(path, ph_native)
            host_phases(path, ph_host)
            rep_native = ph_native.report("  phases, native path")
            rep_host = ph_host.report("  phases, host path")
            lines.append({"walks": walks, "positions": positions, "file_bytes": size, "same_path_data": same,
                          "native_ms": round(native_ms, 2), "host_ms": round(host_ms, 2), "host_over_native": round(host_ms / native_ms, 1),
                          "native_all_ms": [round(x, 2) for x in times[True]], "host_all_ms": [round(x, 2) for x in times[False]],
                          "native_phases_ms": rep_native, "host_phases_ms": rep_host})
    for line in lines:
        say(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(OUT) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
