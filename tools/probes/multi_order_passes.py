"""The level-by-level builder in passes on the headline stream (bench.py's: 10^7 events, 5 * 10^5 nodes).  usage: multi_order_passes.py ROOT TAG MODE
ROOT: the checkout to import pathpyg_amd from (two commits can be compared in one call, alternating processes); TAG: copied into the output.
MODE default : wall ms of from_temporal_graph(K = 3, 5) (bench.py's multi_order headline: 1 warm call, mean of 3)
MODE passes  : K = 5, single pass against PASS_INSTANCES giving about 4 and about 16 parts per level: wall ms and device ms per level
MODE passes16: the build with about 16 parts per level alone (for a kernel trace)
One JSON line per result on stdout (profiles/multi_order_passes.txt)."""
import json
import os
import sys
import time

root, tag, mode = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, root)
import torch  # noqa: E402

import pathpyg_amd as pp  # noqa: E402

assert os.path.realpath(pp.__file__).startswith(os.path.realpath(root)), pp.__file__
dev = "cuda:0"
EVENTS, NODES, SPAN, DELTA = 10_000_000, 500_000, 10_000_000, 1_000_000


def synth_stream(events, nodes, span, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    edge_index = torch.randint(0, nodes, (2, events), generator=g, device=device, dtype=torch.int64)
    time_ = torch.randint(0, span, (events,), generator=g, device=device, dtype=torch.int64)
    return edge_index, time_


def wall(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def emit(rec):
    rec = {"tag": tag, "mode": mode, **rec}
    print(json.dumps(rec), flush=True)


ei, t = synth_stream(EVENTS, NODES, SPAN, 1, dev)
g = pp.TemporalGraph(pp.Data(edge_index=ei, time=t, num_nodes=NODES))
del ei, t

if mode == "default":
    for K in (3, 5):
        ms, mom = wall(lambda: pp.MultiOrderModel.from_temporal_graph(g, delta=DELTA, max_order=K))
        emit({"K": K, "ms": ms, "level_by_level": "layers" in getattr(mom, "sizes", {}), "passes": getattr(mom, "sizes", {}).get("passes")})
        del mom
else:
    from pathpyg_amd import _hip
    from pathpyg_amd.core import multi_order_model as mm
    K = 5
    data = g.data
    base = pp.MultiOrderModel.from_temporal_graph(g, delta=DELTA, max_order=K)
    sizes = base.sizes
    most = max(x[2] for x in sizes["layers"][1:])
    ref = {k: (layer.data.edge_index.clone(), layer.data.edge_weight.clone()) for k, layer in base.layers.items()}
    del base
    plans = [("single", _hip._INT32_ROWS), ("about 4", -(-most // 4)), ("about 16", -(-most // 16))]
    if mode == "passes16":
        plans = plans[2:]
    for name, budget in plans:
        mm.PASS_INSTANCES = budget
        ms, mom = wall(lambda: pp.MultiOrderModel.from_temporal_graph(g, delta=DELTA, max_order=K))
        same = all(torch.equal(mom.layers[k].data.edge_index, ref[k][0]) and torch.equal(mom.layers[k].data.edge_weight, ref[k][1]) for k in ref)
        passes = mom.sizes["passes"]
        del mom
        best = None
        for _ in range(3):
            clock = []
            built = _hip.multi_order_temporal(data.edge_index, data.time, NODES, DELTA, None, K, clock=clock, pass_instances=budget)
            torch.cuda.synchronize()
            per = {}
            for nm, a, b in clock:
                per[nm] = per.get(nm, 0.0) + a.elapsed_time(b)
            if best is None or sum(per.values()) < sum(best.values()):
                best = per
            del built
        emit({"plan": name, "budget": budget, "wall_ms": ms, "passes": passes, "layers": sizes["layers"], "equal_to_single_pass": bool(same),
              "device_ms": {k: round(v, 3) for k, v in best.items()}})
        torch.cuda.empty_cache()
