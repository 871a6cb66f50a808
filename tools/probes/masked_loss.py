"""Masked cross-entropy, forward + backward: pathpyg_amd.nn.cross_entropy(z, y, mask=m) against the torch formulation a training loop on a
node split otherwise runs, F.cross_entropy(z[m], y[m]) — N = 10^6 rows, C = 8, masks of 10 % and 50 %.  The two alternate in one process
after a warm-up; each call is timed with device events; median, quartiles and min - max per row of the table.  One JSON line per mask share."""
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
import pathpyg_amd as pp  # noqa: E402

DEV = "cuda:0"
N, C, WARMUP, REPEATS = 1_000_000, 8, 20, 200


def timed(step):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    step()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main():
    g = torch.Generator(device=DEV).manual_seed(0)
    z = torch.randn(N, C, device=DEV, generator=g).requires_grad_(True)
    y = torch.randint(0, C, (N,), device=DEV, generator=g)
    for share in (0.1, 0.5):
        m = torch.rand(N, device=DEV, generator=g) < share

        def native():
            z.grad = None
            pp.nn.cross_entropy(z, y, mask=m).backward()

        def gather():
            z.grad = None
            F.cross_entropy(z[m], y[m]).backward()

        native()
        mine = z.grad.clone()
        gather()
        assert float((mine - z.grad).abs().max()) <= 1e-5 * float(z.grad.abs().max())
        for _ in range(WARMUP):
            native()
            gather()
        torch.cuda.synchronize()
        times = {"native": [], "gather": []}
        for _ in range(REPEATS):
            times["native"].append(timed(native))
            times["gather"].append(timed(gather))
        row = {"rows": N, "classes": C, "mask_share": share, "selected": int(m.sum())}
        for name, ts in times.items():
            q1, _, q3 = statistics.quantiles(ts, n=4)
            row[name + "_ms"] = {"median": round(statistics.median(ts), 4), "q1": round(q1, 4), "q3": round(q3, 4), "min": round(min(ts), 4),
                                 "max": round(max(ts), 4)}
        row["speedup_median"] = round(row["gather_ms"]["median"] / row["native_ms"]["median"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
