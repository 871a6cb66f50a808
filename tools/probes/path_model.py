"""MultiOrderModel.from_path_data on a device-resident walk store: the level-by-level builder (pp_multiorder_prepare_paths / _step /
_paths_inverse) against the generic kernels (FUSED_BUILDER off) in the same process, alternating, for K = 2..5 — the call, the call plus
reading every layer's four tensors, and estimate_order(max_order=4) — with the per-phase device times of the builder.  Seeded, needs no files.
Both routes' layers are compared tensor by tensor (torch.equal) once before anything is timed.

    python tools/probes/path_model.py [--reps 10] [--shape main|small|both]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pathpyg_amd as pp
from pathpyg_amd import _hip
from pathpyg_amd.core import multi_order_model as mm

DEV = torch.device("cuda:0")
KEYS = ("edge_index", "edge_weight", "node_sequence", "inverse_idx")


def walk_store(n_walks: int, n_nodes: int, seed: int) -> pp.PathData:
    """``n_walks`` random walks of 2..12 nodes on a random graph of ``n_nodes`` nodes with out-degree 8, weights 1..3, as a PathData on the
    device (the tensors PathData.append_walks would have made; node ids are the dense ranks of the nodes that occur)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nbr = torch.randint(0, n_nodes, (n_nodes, 8), generator=g, device=DEV)
    lengths = torch.randint(2, 13, (n_walks,), generator=g, device=DEV)
    cur = torch.randint(0, n_nodes, (n_walks,), generator=g, device=DEV)
    cols = [cur]
    for _ in range(11):
        cur = nbr[cur, torch.randint(0, 8, (n_walks,), generator=g, device=DEV)]
        cols.append(cur)
    grid = torch.stack(cols, dim=1)
    keep = torch.arange(12, device=DEV).unsqueeze(0) < lengths.unsqueeze(1)
    flat = torch.unique(grid[keep], return_inverse=True)[1]
    total = int(flat.numel())
    last = torch.zeros(total, dtype=torch.bool, device=DEV)
    last[torch.cumsum(lengths, 0) - 1] = True
    tails = torch.arange(total, device=DEV)[~last]
    paths = pp.PathData(pp.IndexMap(list(range(int(flat.max()) + 1))), device=DEV)      # (estimate_order compares the node ids of walks and model)
    d = paths.data
    d.edge_index = torch.stack((tails, tails + 1))
    d.node_sequence = flat.unsqueeze(1)
    d.dag_weight = torch.randint(1, 4, (n_walks,), generator=g, device=DEV).float()
    d.dag_num_edges = lengths - 1
    d.dag_num_nodes = lengths
    d.num_nodes = total
    return paths


def build(paths, K, fused, read=False, order=False):
    mm.FUSED_BUILDER = fused
    try:
        model = pp.MultiOrderModel.from_path_data(paths, max_order=K)
        if read:
            for layer in model.layers.values():
                for key in KEYS:
                    layer.data[key]
        if order:
            model.estimate_order(paths, max_order=K)
    finally:
        mm.FUSED_BUILDER = True
    return model


def timed(paths, K, reps, **kw):
    """ms of ``reps`` runs of both routes, alternating, after one warm-up each: {route: [ms]}"""
    out = {True: [], False: []}
    for it in range(reps + 1):
        for fused in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            build(paths, K, fused, **kw)
            torch.cuda.synchronize()
            if it:
                out[fused].append(1e3 * (time.perf_counter() - t0))
    return out


def line(what, ms):
    new, old = ms[True], ms[False]
    med_new, med_old = statistics.median(new), statistics.median(old)
    return (f"{what:<34} level-by-level {med_new:8.2f} ms [{min(new):.2f} .. {max(new):.2f}]   generic {med_old:8.2f} ms [{min(old):.2f} .. {max(old):.2f}]"
            f"   x{med_old / med_new:.2f}   {'faster by more than the spread' if max(new) < min(old) else 'NOT separated by the spread'}")


def probe(name, paths, reps):
    d = paths.data
    n = int(d.node_sequence.max()) + 1
    print(f"== {name}: {d.dag_num_nodes.numel()} walks, {d.node_sequence.size(0)} positions, {d.edge_index.size(1)} edges, {n} nodes", flush=True)
    fast, slow = build(paths, 5, True), build(paths, 5, False)
    took = "layers" in getattr(fast, "sizes", {})
    print(f"level-by-level route taken at K = 5: {took}" + ("" if took else "  (a type with more than 4096 children, or another refusal: both columns below are the generic kernels)"))
    assert "layers" not in getattr(slow, "sizes", {})
    for k in range(1, 6):
        for key in KEYS:
            assert torch.equal(fast.layers[k].data[key], slow.layers[k].data[key]), (k, key)
    if took:
        print("layers (nodes, edges, instances): " + ", ".join(str(s) for s in fast.sizes["layers"]))
    print("both routes' layers 1..5 are equal, tensor by tensor", flush=True)
    del fast, slow
    for K in range(2, 6):
        print(line(f"K = {K}: the call", timed(paths, K, reps)), flush=True)
        print(line(f"K = {K}: call + all tensors read", timed(paths, K, reps, read=True)), flush=True)
    print(line("K = 4: call + estimate_order(4)", timed(paths, 4, reps, order=True)), flush=True)
    for K in range(2, 6):
        for _ in range(2):
            clock = []
            _hip.multi_order_paths(d.node_sequence, d.dag_num_nodes, d.dag_weight, d.edge_index, n, K, clock=clock)
            torch.cuda.synchronize()
        print(f"K = {K} phases (device ms): " + ", ".join(f"{what} {a.elapsed_time(b):.3f}" for what, a, b in clock), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", default="both", choices=("main", "small", "both"))
    args = ap.parse_args()
    print(f"{torch.cuda.get_device_name(0)}; times are host wall clock around a synchronise, median [min .. max] of {args.reps} runs, routes alternating")
    if args.shape in ("main", "both"):
        probe("main shape", walk_store(1_000_000, 10_000, 1), args.reps)
    if args.shape in ("small", "both"):
        probe("second shape", walk_store(200_000, 300, 2), args.reps)
