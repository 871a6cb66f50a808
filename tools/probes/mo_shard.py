"""The De Bruijn layers 1..5 of the headline stream (BASELINE configs[4]) on 8 EMULATED ranks (threads of one process on one GPU, ThreadWorld,
"events" clock), split by first node: per rank and level the device time of the rank's turns, the instances it owns and the bytes of the
all-gathers; beside them the single-GPU ``MultiOrderModel.from_temporal_graph(max_order=5)`` call, alternating, after a warm-up.

    python tools/probes/mo_shard.py [--ranks 8] [--rounds 2] [--baseline-root DIR]

``--baseline-root``: a checkout of another commit (built) whose single-GPU call is measured too, in a process of its own, in the same rounds.
Eight ranks on one device are not a scaling curve: they share the memory system and run one after the other."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
M, N, SPAN, DELTA, K = 10_000_000, 500_000, 10_000_000, 1_000_000, 5
DEV = "cuda:0"


def stream(pp, torch):
    g = torch.Generator(device=DEV).manual_seed(0)
    ei = torch.randint(0, N, (2, M), generator=g, device=DEV)
    t = torch.randint(0, SPAN, (M,), generator=g, device=DEV)
    return pp.TemporalGraph(pp.Data(edge_index=ei, time=t, num_nodes=N))


def single(root: str, calls: int = 3) -> list:
    """ms of ``from_temporal_graph(K)`` calls (after one warm-up) with the package found under ``root``, in a fresh process."""
    code = (
        "import sys, time, json, torch; sys.path.insert(0, %r)\n"
        "import pathpyg_amd as pp\n"
        "sys.path.insert(0, %r)\n"
        "from tools.probes.mo_shard import stream, DELTA, K\n"
        "tg = stream(pp, torch); out = []\n"
        "for it in range(%d):\n"
        "    torch.cuda.synchronize(); t0 = time.perf_counter()\n"
        "    mom = pp.MultiOrderModel.from_temporal_graph(tg, delta=DELTA, max_order=K)\n"
        "    torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)\n"
        "    assert 'layers' in getattr(mom, 'sizes', {}); del mom\n"
        "print('MS ' + json.dumps(out[1:]))\n" % (root, ROOT, calls + 1))
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, cwd=root)
    if done.returncode != 0:
        raise RuntimeError(done.stderr[-2000:])
    return json.loads(next(line for line in done.stdout.splitlines() if line.startswith("MS "))[3:])


def sharded(ranks: int, tg, warm: bool):
    import torch
    from pathpyg_amd import distributed as pd

    def body(comm):
        comm.tw.take_turn(comm)          # a rank starts when the baton reaches it: its windows pass runs (and is timed) alone
        comm.trace = {}
        comm.reset_counters()
        shard = pd.build_multi_order_shard(tg, DELTA, K, comm)
        assert shard is not None
        comm.end_turns()
        trace = comm.resolve_trace()
        gathers = [b for kind, b, _ in comm.events if kind == "all_gather"]
        return {"ms": {k: v * 1e3 for k, v in trace.items()}, "total_ms": comm.compute_s * 1e3, "host_ms": comm.host_s * 1e3,
                "instances": [e.n_instances for e in shard.layers], "rows": [e.row_hi - e.row_lo for e in shard.layers],
                "edges": [int(e.col.numel()) for e in shard.layers], "sizes": [(e.n_nodes, e.n_edges) for e in shard.layers],
                "gather_block_bytes": gathers, "sent_all_gather": comm.sent_bytes["all_gather"]}

    out = pd.run_thread_world(ranks, body, device=DEV, clock="events")
    torch.cuda.synchronize()
    return None if warm else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--baseline-root", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import pathpyg_amd as pp
    tg = stream(pp, torch)
    sharded(args.ranks, tg, warm=True)
    report = {"rounds": []}
    for _ in range(args.rounds):
        entry = {}
        if args.baseline_root:
            entry["single_gpu_baseline_ms"] = single(args.baseline_root)
        entry["single_gpu_ms"] = single(ROOT)
        t0 = time.perf_counter()
        entry["ranks"] = sharded(args.ranks, tg, warm=False)
        entry["sharded_wall_ms"] = (time.perf_counter() - t0) * 1e3
        report["rounds"].append(entry)
    last = report["rounds"][-1]
    ranks = last["ranks"]
    labels = ["mo windows"] + [f"mo level {k}" for k in range(1, K + 1)]
    print("| rank | " + " | ".join(f"{label[3:]} ms" for label in labels) + " | total ms | without windows | instances per level |")
    print("|---|" + "---|" * (len(labels) + 3))
    for r, e in enumerate(ranks):
        ms = [e["ms"].get(label, 0.0) for label in labels]
        print(f"| {r} | " + " | ".join(f"{v:.2f}" for v in ms) + f" | {sum(ms):.2f} | {sum(ms[1:]):.2f} | {e['instances']} |")
    sizes = ranks[0]["sizes"]
    print("\n| level | U_k | A_k | formula 4 (U_k + 1) + 4 A_k | gathered (ranks x padded block) | per-rank block |")
    print("|---|---|---|---|---|---|")
    for k, block in enumerate(ranks[0]["gather_block_bytes"], start=1):
        u, a = sizes[k - 1]
        print(f"| {k} | {u} | {a} | {4 * (u + 1) + 4 * a} | {block * args.ranks} | {block} |")
    for i, e in enumerate(report["rounds"]):
        slow = max(sum(x["ms"].values()) for x in e["ranks"])
        slow_nw = max(sum(v for k, v in x["ms"].items() if k != "mo windows") for x in e["ranks"])
        print(f"round {i}: single GPU {e['single_gpu_ms']} ms" + (f", baseline commit {e['single_gpu_baseline_ms']} ms" if args.baseline_root else "") +
              f"; slowest rank {slow:.2f} ms, without the replicated windows pass {slow_nw:.2f} ms; host wall of the emulation {e['sharded_wall_ms']:.0f} ms")
    print("JSON " + json.dumps(report))


if __name__ == "__main__":
    main()
