"""One build at real size: a stream whose TOP level alone has 2^31 or more instances.  usage: multi_order_real_size.py probe|build
probe: K = 2 (sizes and time of the level below);  build: K = 3 with the default budget and with PASS_INSTANCES = 2^30, compared.
Few nodes on purpose: 215^4 < 2^31 keeps the top layer's EDGES below the int32 limit while its instances pass it, and
215^2 node pairs keep every type below 4096 children.  One JSON line per result on stdout (profiles/multi_order_passes.txt)."""
import json
import pathlib
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))

import pathpyg_amd as pp
from pathpyg_amd.core import multi_order_model as mm

mode = sys.argv[1]
dev = "cuda:0"
M, N, SPAN, DELTA = 6_500_000, 215, 100_000_000, 62_000


def emit(rec):
    print(json.dumps({"mode": mode, **rec}), flush=True)


free, total = torch.cuda.mem_get_info()
emit({"free_GB": free / 1e9, "total_GB": total / 1e9})
if free < 100e9:
    emit({"skipped": "less than 100 GB free"})
    sys.exit(0)
gen = torch.Generator(device=dev).manual_seed(7)
src = torch.randint(0, N, (M,), generator=gen, device=dev)
dst = torch.randint(0, N, (M,), generator=gen, device=dev)
t = torch.randint(0, SPAN, (M,), generator=gen, device=dev)
g = pp.TemporalGraph(pp.Data(edge_index=torch.stack((src, dst)), time=t, num_nodes=N))
del src, dst, t


def build(K, budget):
    mm.PASS_INSTANCES = budget
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    model = pp.MultiOrderModel.from_temporal_graph(g, delta=DELTA, max_order=K)
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    assert "layers" in getattr(model, "sizes", {}), "the level-by-level builder handed the stream back"
    return model, s, torch.cuda.max_memory_allocated() / 1e9


def csr(model, k):
    b = mm._builder_csr(model.layers[k])
    assert b is not None
    return b


def checks(model, K):
    out = {}
    for k in range(1, K + 1):
        b = csr(model, k)
        a = b.n_edges
        weight_sum = float(b.weight[:a].double().sum())
        ptr = b.row_ptr[:b.n_nodes + 1].long()
        starts = torch.zeros(a + 1, dtype=torch.bool, device=dev)
        starts[ptr] = True
        col = b.col[:a]
        ascending = bool(((col[1:] > col[:-1]) | starts[1:a]).all()) and bool((ptr[1:] >= ptr[:-1]).all()) and int(ptr[0]) == 0 and int(ptr[-1]) == a
        out[k] = {"instances": b.n_instances, "weight_sum_f64": weight_sum, "sum_equals_instances": weight_sum == float(b.n_instances),
                  "edge_index_lexicographically_sorted": ascending}
        del starts, ptr
    return out


if mode == "probe":
    # (from_temporal_graph(max_order=2) runs the order-2 builder: the level below the top is taken from the level-by-level builder itself)
    from pathpyg_amd import _hip
    data = g.data
    for _ in range(2):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        built = _hip.multi_order_temporal(data.edge_index, data.time, N, DELTA, None, 2)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
    assert built is not None, "the level-by-level builder handed the stream back"
    emit({"K": 2, "m": M, "n": N, "delta": DELTA, "span": SPAN, "seconds": s, "peak_GB": torch.cuda.max_memory_allocated() / 1e9,
          "layers": [(b.n_nodes, b.n_edges, b.n_instances) for b in built]})
else:
    first, s1, peak1 = build(3, mm._INT32_ROWS)
    emit({"K": 3, "m": M, "n": N, "delta": DELTA, "span": SPAN, "budget": mm._INT32_ROWS, "seconds": s1, "peak_GB": peak1, "layers": first.sizes["layers"],
          "passes": first.sizes["passes"], "checks": (verdict := checks(first, 3))})
    assert first.sizes["layers"][2][2] >= 1 << 31, "the top level was meant to have 2^31 or more instances"
    assert all(v["sum_equals_instances"] and v["edge_index_lexicographically_sorted"] for v in verdict.values()), verdict
    second, s2, peak2 = build(3, 1 << 30)
    same = all(torch.equal(getattr(csr(first, k), name)[:n], getattr(csr(second, k), name)[:n])
               for k in (1, 2, 3) for name, n in (("row_ptr", csr(first, k).n_nodes + 1), ("col", csr(first, k).n_edges), ("weight", csr(first, k).n_edges)))
    emit({"K": 3, "budget": 1 << 30, "seconds": s2, "peak_GB": peak2, "layers": second.sizes["layers"], "passes": second.sizes["passes"],
          "bit_equal_to_the_first_build": bool(same), "passes_differ": second.sizes["passes"] != first.sizes["passes"]})
    assert same and second.sizes["passes"] != first.sizes["passes"] and second.sizes["layers"] == first.sizes["layers"]
