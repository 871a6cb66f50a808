"""Two measurements behind DESIGN.md's section on the partitioned semi-supervised loop, one JSON line each.

A. The first GCN layer on implicit one-hot features, forward + backward on ONE order-2 shard of the benchmark's stream (10^7 events, 5 * 10^5
   nodes, delta 10^6, F = 64): the row-mapped kernel (pp_spmm_diag_drop_map_f32) against the composition of the pre-existing kernels (gather
   W^T[rows], scale, pp_spmm_f32; pp_spmm_f32, scale, index_add_) — the two alternate in one process after a warm-up, each call between two
   device events; p = 0 and p = 0.4.  ``--ranks 1``: the whole graph as one shard (identity map); ``--ranks R``: the shard of rank 1 of R
   emulated ranks (node-range partition: owned rows in send order + halo rows, a non-monotone map).
B. ``ShardedDBGNN.loss``: the loss part of a step (forward + backward on the rank's logits) with the keyword-free mean against the masked,
   weighted mean with its all-reduce, on R emulated ranks holding the benchmark's rows (5 * 10^5 / R each, 8 classes).  Every iteration of both
   ends in a barrier, so both pay the same turn; the ranks' compute clocks (``Comm.lap``) give the time per call."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402
from pathpyg_amd import distributed as pd  # noqa: E402
from pathpyg_amd.nn.sharded import HipOps, _ShardedMaskedLoss  # noqa: E402

DEV = torch.device("cuda:0")


def timed(step):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    step()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def summary(ts):
    q1, _, q3 = statistics.quantiles(ts, n=4)
    return {"median": round(statistics.median(ts), 4), "q1": round(q1, 4), "q3": round(q3, 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def first_layer(gs, f, warmup, repeats):
    plan, rows, n = gs.plan, gs.rows, gs.num_nodes
    gen = torch.Generator(device=DEV).manual_seed(0)
    wt = torch.randn(n, f, device=DEV, generator=gen) * 0.05
    bias = torch.zeros(f, device=DEV)
    dpre = torch.randn(plan.n_dst, f, device=DEV, generator=gen)
    out = torch.empty(plan.n_dst, f, device=DEV)
    row = {"what": "one-hot first layer fwd + bwd", "n": n, "n_own": plan.n_dst, "n_src": plan.n_src, "entries": int(plan.fwd_idx.numel()), "F": f,
           "map_is_identity": bool(torch.equal(rows, torch.arange(rows.numel(), device=DEV)))}
    for p in (0.0, 0.4):
        site = None if p == 0 else (p, 12345, 64)

        def run(fused):
            HipOps.ONE_HOT_FUSED = fused
            HipOps.one_hot_forward(plan, wt, bias, rows, n, site, out)
            return HipOps.one_hot_backward(plan, dpre, rows, n, site)

        a, ya = run(True), out.clone()
        b = run(False)
        assert float((ya - out).abs().max()) <= 1e-5 * float(out.abs().max()) and float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
        del a, b, ya
        for _ in range(warmup):
            run(True)
            run(False)
        torch.cuda.synchronize()
        times = {"fused": [], "composition": []}
        for _ in range(repeats):
            times["fused"].append(timed(lambda: run(True)))
            times["composition"].append(timed(lambda: run(False)))
        row[f"p{p}"] = {k: summary(v) for k, v in times.items()}
        row[f"p{p}"]["composition_over_fused"] = round(statistics.median(times["composition"]) / statistics.median(times["fused"]), 3)
    HipOps.ONE_HOT_FUSED = True
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=10_000_000)
    ap.add_argument("--nodes", type=int, default=500_000)
    ap.add_argument("--span", type=int, default=10_000_000)
    ap.add_argument("--delta", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--loss-ranks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--skip-layer", action="store_true")
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(1)
    if not args.skip_layer:
        ei = torch.randint(0, args.nodes, (2, args.events), generator=gen).to(DEV)
        t = torch.sort(torch.randint(0, args.span, (args.events,), generator=gen)).values.to(DEV)
        tg = pp.TemporalGraph(pp.Data(edge_index=ei, time=t, num_nodes=args.nodes))
        y = torch.zeros(args.nodes, dtype=torch.int64, device=DEV)
        if args.ranks == 1:
            shard = pd.build_dbgnn_shard(tg, args.delta, None, None, y, pd.Comm())
            print(json.dumps(first_layer(shard.ho, args.features, args.warmup, args.repeats)), flush=True)
        else:
            def body(comm):
                shard = pd.build_dbgnn_shard(tg, args.delta, None, None, y, comm)
                comm.barrier()
                row = first_layer(shard.ho, args.features, args.warmup, args.repeats) if comm.rank == 1 else None
                comm.barrier()
                return row
            print(json.dumps(dict(pd.run_thread_world(args.ranks, body, DEV)[1], ranks=args.ranks, rank=1)), flush=True)

    # ---- B
    world, classes, calls = args.loss_ranks, 8, 50
    n_own = args.nodes // world
    weight = (torch.rand(classes, generator=gen) + 0.5).to(DEV)

    def loss_body(comm):
        g = torch.Generator(device=DEV).manual_seed(comm.rank)
        z = torch.randn(n_own, classes, device=DEV, generator=g).requires_grad_(True)
        y_own = torch.randint(0, classes, (n_own,), device=DEV, generator=g)
        mask = torch.rand(n_own, device=DEV, generator=g) < 0.5
        ops = HipOps()

        def plain():
            z.grad = None
            (ops.cross_entropy_mean(z, y_own) * (n_own / args.nodes)).backward()

        def masked():
            z.grad = None
            _ShardedMaskedLoss.apply(z, y_own, mask, weight, -1, True, comm, ops)[0].backward()

        out = {}
        for name, fn in (("plain", plain), ("masked", masked), ("plain_again", plain), ("masked_again", masked)):
            for _ in range(5):
                fn()
                comm.barrier()
            a = comm.lap()
            for _ in range(calls):
                fn()
                comm.barrier()
            out[name] = comm.between(a, comm.lap()) / calls * 1e3
        return out

    ranks = pd.run_thread_world(world, loss_body, DEV)
    row = {"what": "loss part of a step per rank, ms per call (fwd + bwd)", "ranks": world, "rows_per_rank": n_own, "classes": classes}
    for name in ranks[0]:
        row[name] = summary([r[name] for r in ranks])
    row["extra_ms_median"] = round(statistics.median([(r["masked"] + r["masked_again"] - r["plain"] - r["plain_again"]) / 2 for r in ranks]), 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
