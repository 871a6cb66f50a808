#!/usr/bin/env python3
"""Headline benchmark: k=2 De Bruijn lift of a synthetic temporal edge stream + one DBGNN train step, on 1..N MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the headline line (with the per-kernel figures of the timed steps themselves).
``--full`` adds everything measured outside the timed steps: the generic-kernel lift / aggregation / line-graph rooflines, the step through the
reference API, the hub streams, the multi-order builds and the CPU baseline.  ``--dump-outputs DIR`` writes what the last timed step computed
(loss, weights after the update, their gradients, seeded samples of both layers' GCN plans) as DIR/<name>.npy.

``--gpus N`` with N > 1 and no RANK in the environment re-launches itself under ``torch.distributed.run`` (one process per GPU,
backend nccl = RCCL over xGMI, rendezvous on 127.0.0.1); when the driver already started it that way the ranks are taken from the
environment.  One STEP = one pass of the hot path over the synthetic events, which are already resident (replicated) in HBM:

  partition (default, the north-star split; "scaling": "strong" — ONE global stream whatever N is):
      layer 1 -> edge-range sharded event-graph lift -> lifted pairs to the owner of their destination (one all-to-all) -> coalesce
      -> graph shards (halo, rectangular GCN plans) -> destination-partitioned DBGNN forward / loss / backward with one embedding
      exchange per layer, reduce-scatter of the bipartite partial sums, all-reduce of the weight gradients -> Adam
      (pathpyg_amd.distributed.build_dbgnn_shard + pathpyg_amd.nn.sharded.ShardedDBGNN; at N = 1 every collective is the identity)
  streams (--mode streams; "scaling": "weak"): every rank runs the single-GPU API path
      (MultiOrderModel.from_temporal_graph + to_dbgnn_data + DBGNN) on its own stream; only weight gradients are all-reduced.

Workload (SURVEY.md §8d "10M temporal edges" headline of BASELINE.json): temporal ER stream, m = 10^7 events, N = 5*10^5 nodes,
int64 timestamps uniform in [0, 10^7), delta = 10^6 (E2 ~ 1.9*10^7), 64-dim features, hidden_dims [64, 64, 64], 8 classes, fp32.
The JSON line follows the driver's contract and adds `roofline` (the most expensive (kernel, graph) pair, live HIP-event timing),
`kernel_rooflines` (every timed kernel per graph), and with --full `lift_roofline` / `aggregation_roofline` (SURVEY §8d bytes over the
whole lift / aggregation incl. their sorts and scans), `api_path`, `hub_streams`, `multi_order` and `cpu_baseline` (BASELINE.md §3
protocol, bounded).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak (guide: MI355X_MICROARCH.md); ~6300 GB/s is what a copy achieves


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--events", type=int, default=10_000_000, help="temporal edges of the stream (partition: global; streams: per GPU)")
    ap.add_argument("--nodes", type=int, default=500_000)
    ap.add_argument("--span", type=int, default=10_000_000)
    ap.add_argument("--delta", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--dropout", type=float, default=0.0, help="p_dropout of the model (the headline number is quoted at 0; the reference's own test uses 0.4)")
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--mode", choices=("auto", "partition", "streams"), default="auto",
                    help="auto: the north-star partition at 1 GPU and from 8 GPUs on; at 2..7 GPUs `streams` (independent streams, weak scaling) — "
                         "xGMI is point-to-point, so a rank's halo (7/8 of its order-2 source rows on an ER stream, whatever the cut) crosses W-1 links: "
                         "640 MB per layer exchange on ONE link at 2 ranks, 160 MB at 4, 40 MB at 8; the projections (profiles/r04_shapes/emulate{2,4}.json) "
                         "put the 2- and 4-rank partition step at 42.7 / 14.8 ms against 14.0 ms on one GPU: reported as what it is, not as scaling")
    ap.add_argument("--no-hub-streams", action="store_true", help="skip the builder timings on the two hub streams (hub_streams in the line)")
    ap.add_argument("--no-multi-order", action="store_true", help="skip the K = 2..5 / K = 1..3 multi-order builds (multi_order in the line)")
    ap.add_argument("--no-api-path", action="store_true", help="skip the extra (untimed for `value`) steps through the reference API that fill api_path_ms_per_step")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help="gloo: host-staged collectives (tests; several ranks may share one GPU)")
    ap.add_argument("--share-gpu", action="store_true", help="all ranks use cuda:0 (single-GPU test boxes, with --backend gloo)")
    ap.add_argument("--emulate-ranks", type=int, default=0, help="run R ranks of the partition path as R threads on ONE GPU, taking turns: per-rank "
                                                                 "compute time + bytes per xGMI link of every collective -> a LABELLED PROJECTION of the "
                                                                 "R-GPU step (not a measurement of R GPUs; prints its own JSON report)")
    ap.add_argument("--emulate-clock", choices=("events", "drain"), default="events",
                    help="--emulate-ranks: how a rank's turns are timed. events: two stream events per turn, nothing drained at the collectives, per rank "
                         "max(device, host) (what a stream-ordered RCCL run pays); drain: GPU drained at the end of every turn (upper bound)")
    ap.add_argument("--trace", action="store_true", help="--emulate-ranks: per-phase compute time of rank 1 in the report")
    ap.add_argument("--host-profile", default="", help="--emulate-ranks: cProfile of rank 1's timed steps, written to this file (the host side of a "
                                                       "rank-step; waiting for the other ranks' turns shows up as lock acquires)")
    ap.add_argument("--no-overlap", action="store_true", help="partition path without the interleaved exchange schedule (A/B)")
    ap.add_argument("--fo-halo", choices=("auto", "dense", "discovered"), default="auto", help="partition path, world > 1: halo of the first-order shard "
                    "(dense = every foreign node, no discovery round; auto picks it when a rank's in-edges exceed 1.5 x the node count)")
    ap.add_argument("--halo-row-backward", action="store_true", help="partition path, world > 1: the round-2 backward (fused kernel over owned + halo rows, "
                    "its output exchanged) instead of exchanging A^T dpre and multiplying on the owned rows only (A/B)")
    ap.add_argument("--builder", choices=("fused", "generic"), default="fused", help="1 GPU: graph construction by the node-by-node order-2 builder "
                    "(pp_debruijn2_*; one read-back, the event graph is never written) or by the generic kernels (lift -> coalesce -> plans)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-loop-events", type=int, default=6_000, help="smallest of the three B-loop sizes (x2, x4 follow; kept below torch's 32768-element parallel grain)")
    ap.add_argument("--cpu-sample-events", type=int, default=10_000_000, help="size of the vectorised CPU pipeline legs (B-agg, B-dbgnn): the FULL workload by "
                                                                                "default (BASELINE.md §3: full size where host RAM allows; capped at --events)")
    ap.add_argument("--cpu-baseline-only", action="store_true", help="run only the CPU baseline and print its JSON (used by the main run, in a "
                                                                      "subprocess with a hard time limit, so that it can never stall the bench line)")
    ap.add_argument("--cpu-baseline-timeout", type=int, default=1200)
    ap.add_argument("--full", action="store_true", help="also measure what lies outside the timed steps (generic-kernel rooflines, API path, hub "
                                                        "streams, multi-order builds, line-graph lift, CPU baseline); a plain run does none of it")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, "
                                                                      "large arrays as a fixed seeded sample, < 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


class ResidentRows:
    """Row store of a partitioned run: a rank's OWNED feature rows are resident (placed once, in a buffer with room for the halo rows behind
    them), only the halo rows — whatever the current graph makes them — are fetched per step.  `full` stands in for the other ranks' stores (in
    the emulation and in this bench every process can read the whole matrix; a sharded deployment fetches the halo rows over xGMI instead)."""

    def __init__(self, full: torch.Tensor):
        self.full = full
        self.placed = {}          # (lo, hi) -> buffer [n_own + halo capacity, F]; one entry per rank (threads of the emulation share the object)

    def shard_rows(self, lo: int, hi: int, halo_ids: torch.Tensor | None) -> torch.Tensor:
        n_own, n_halo = hi - lo, 0 if halo_ids is None else int(halo_ids.numel())
        buf = self.placed.get((lo, hi))
        if buf is None or buf.size(0) < n_own + n_halo:
            buf = torch.empty((n_own + n_halo + n_halo // 8 + 1, self.full.size(1)), dtype=self.full.dtype, device=self.full.device)
            buf[:n_own] = self.full[lo:hi]                     # placement of the owned rows: once per ownership range
            self.placed[(lo, hi)] = buf
        if n_halo:
            torch.index_select(self.full, 0, halo_ids, out=buf[n_own: n_own + n_halo])
        return buf[: n_own + n_halo]

    def shard_rows_static(self, lo: int, hi: int, halo_ids: torch.Tensor) -> torch.Tensor:
        """Rows of a DENSE-halo shard (halo = every foreign node, the same set at every step): fetched once, kept with the owned rows."""
        key = ("static", lo, hi, int(halo_ids.numel()))
        buf = self.placed.get(key)
        if buf is None:
            buf = torch.cat((self.full[lo:hi], self.full.index_select(0, halo_ids)))
            self.placed[key] = buf
        return buf

    def rows_buffer(self, lo: int, hi: int, row_of: torch.Tensor, n_halo: int) -> torch.Tensor:
        """[n_own + n_halo, F] with the owned rows lo + row_of in front (the LOCAL row order of a node-range shard, which follows this step's
        graph: one row gather per step), room for the halo rows, which arrive by exchange (pathpyg_amd.distributed._build_partitioned_by_node)."""
        from pathpyg_amd import _hip
        n_own = hi - lo
        buf = self.placed.get(("rows", lo, hi))
        if buf is None or buf.size(0) < n_own + n_halo:
            buf = torch.empty((n_own + n_halo + n_halo // 8 + 1, self.full.size(1)), dtype=self.full.dtype, device=self.full.device)
            self.placed[("rows", lo, hi)] = buf
        if n_own:
            _hip.gather_rows(self.full[lo:hi], row_of, out=buf[:n_own])
        return buf[: n_own + n_halo]

    def __call__(self, rows: torch.Tensor) -> torch.Tensor:      # (plain row-loader form, world size 1 / callers without a shard)
        return self.full.index_select(0, rows)


def synth_stream(events: int, nodes: int, span: int, seed: int, device):
    """Temporal Erdos-Renyi stream: endpoints and timestamps i.i.d. uniform (self loops kept), unsorted."""
    g = torch.Generator(device=device).manual_seed(seed)
    edge_index = torch.randint(0, nodes, (2, events), generator=g, device=device, dtype=torch.int64)
    time_ = torch.randint(0, span, (events,), generator=g, device=device, dtype=torch.int64)
    return edge_index, time_


# ---------------------------------------------------------------------------------------------------------------------------------
# live kernel timing: HIP events around C-ABI entry points on the stream they launch on
class KernelClock:
    """HIP events around every call of one C-ABI entry point; with `until` (one name or several): around the call of `name` (the count
    phase) AND around the following call of each `until` entry point in turn (count / fill phases) — separate intervals, because count phases
    of independent operations are queued together and other kernels run between an operation's phases."""

    def __init__(self, lib, name: str, describe, until=None):
        self.lib, self.name, self.describe = lib, name, describe
        # (a phase may be entered through either of several entry points: a tuple of names — pp_debruijn2_fill / pp_debruijn2_fill_ready)
        phases = [until] if isinstance(until, str) else list(until or [])
        self.until = [(k, u) for k, names in enumerate(phases) for u in ((names,) if isinstance(names, str) else names)]
        self.n_phases = len(phases)
        self.orig = getattr(lib, name)
        self.orig_until = [getattr(lib, u) for _, u in self.until]
        self.records = []          # ([(start_event, end_event), ...], key, bytes)
        self.enabled = False
        self._open = None

    @staticmethod
    def _timed(fn, args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        rc = fn(*args)
        e1.record(torch.cuda.current_stream())
        return rc, e0, e1

    def __enter__(self):
        def wrapped(*args):
            if not self.enabled:
                return self.orig(*args)
            rc, e0, e1 = self._timed(self.orig, args)
            if not self.until:
                self.records.append(([(e0, e1)],) + tuple(self.describe(*args)))
            else:
                self._open = ([(e0, e1)],) + tuple(self.describe(*args))
            return rc
        setattr(self.lib, self.name, wrapped)
        for (k, name), orig in zip(self.until, self.orig_until):
            def wrapped_until(*args, _k=k, _orig=orig):
                if not (self.enabled and self._open is not None and len(self._open[0]) == _k + 1):
                    return _orig(*args)
                rc, f0, f1 = self._timed(_orig, args)
                self._open[0].append((f0, f1))
                if _k + 1 == self.n_phases:
                    self.records.append(self._open)
                    self._open = None
                return rc
            setattr(self.lib, name, wrapped_until)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)
        for (_, name), orig in zip(self.until, self.orig_until):
            setattr(self.lib, name, orig)

    def groups(self) -> dict:
        """{key: (launches, total ms, total algorithmic bytes)}"""
        out = {}
        for intervals, key, nbytes in self.records:
            n, ms, b = out.get(key, (0, 0.0, 0))
            out[key] = (n + 1, ms + sum(e0.elapsed_time(e1) for e0, e1 in intervals), b + nbytes)
        return out


CSR_SHAPE = {}          # idx.data_ptr() of a CSR -> number of entries (registered when plans are built; the kernels only see pointers)


def register_plan(plan) -> None:
    for idx in (plan.fwd_idx, plan.bwd_idx):
        if idx is not None:
            CSR_SHAPE[idx.data_ptr()] = int(idx.numel())


def _rows_label(n: int) -> str:
    return f"{n:.2e} rows"


def spmm_desc(ptr, idx, val, n_rows, x, f, self_coef, s, bias, act, heavy_slot, heavy_sum, y, stream):
    """pp_spmm_f32: CSR once, every source row once (the bench registers the source-row count with the plan; at most one
    row per CSR entry), every output row once (+ the self-term rows when they are a separate matrix)."""
    nnz = CSR_SHAPE.get(idx, 0)
    n_src = SRC_ROWS.get(idx, nnz)
    total = 4 * (n_rows + 1) + nnz * (4 + (4 if val else 0)) + 4 * f * (min(n_src, nnz) + n_rows)
    if self_coef:
        total += 4 * n_rows + (4 * f * n_rows if (s and s != x) else 0)
    return (f"k_spmm_v4 (pp_spmm_f32) F={f}, {_rows_label(n_rows)}", total)


SRC_ROWS = {}           # idx.data_ptr() -> rows of the matrix the CSR gathers from


def gcn_forward_desc(ptr, idx, val, n_rows, n_src, x, p, self_coef, w, q, bias, act, heavy_slot, heavy_sum, agg_out, y, *drop_and_stream):
    """pp_gcn_forward_f32: CSR once, every input row once (P wide), every output row once (Q wide), the optional aggregated-input copy,
    the self coefficients and W."""
    nnz = CSR_SHAPE.get(idx, 0)
    total = (4 * (n_rows + 1) + nnz * (4 + (4 if val else 0)) + 4 * p * n_src + 4 * q * n_rows + (4 * n_rows if self_coef else 0)
             + (4 * p * n_rows if agg_out else 0) + 4 * p * q)
    return (f"k_gcn_forward<{p},{q}> (pp_gcn_forward_f32), {_rows_label(n_rows)}", total)


def gcn_backward_desc(ptr, idx, val, n_rows, n_self, nnz_hint, d, m, self_coef, x, k, w, fuse_act, heavy_slot, heavy_sum, d_in, colsum, dw, ws, ws_bytes,
                      *drop_and_stream):
    """pp_gcn_backward_f32: CSR, dpre (M wide) and the layer input (K wide) read once, the input gradient (K wide) written once."""
    nnz = CSR_SHAPE.get(idx, 0)
    total = 4 * (n_rows + 1) + nnz * (4 + (4 if val else 0)) + 4 * m * n_self + 8 * k * n_rows + (4 * n_self if self_coef else 0) + 8 * m * k
    return (f"k_gcn_backward<{m},{k}> (pp_gcn_backward_f32), {_rows_label(n_rows)}", total)


def pmc_traffic(kernel_key: str, args) -> float | None:
    """HBM bytes per launch of a (kernel, graph) pair from the committed rocprofv3 --pmc passes (profiles/, separate FETCH_SIZE and
    WRITE_SIZE runs of this same command, gfx950 FETCH correction applied).  Only valid for the default workload at 1 GPU."""
    pmc_traffic.source = None
    defaults = (10_000_000, 500_000, 10_000_000, 1_000_000, 64)
    if (args.events, args.nodes, args.span, args.delta, args.features) != defaults:
        return None
    for name in PMC_TABLES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as fh:
                table = json.load(fh)
            short = kernel_key.split(" ")[0].split("<")[0]
            big = kernel_key.endswith("1.00e+07 rows")
            for key in ((short + ("@ho" if big else "@fo")), short):          # (kernels launched on one graph only have no @ split)
                if key in table:
                    pmc_traffic.source = "profiles/" + name
                    return float(table[key]["hbm_bytes_per_dispatch"])
        except (OSError, KeyError, ValueError):
            continue
    return None


PMC_TABLES = ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json")
pmc_traffic.source = None


# ---------------------------------------------------------------------------------------------------------------------------------
def cpu_baseline(args, seed: int) -> dict:
    """BASELINE.md §3 / SURVEY §8(d) CPU protocol on this box's host cores, bounded to ~30-40 s:
      B-loop   : the oracle's op-for-op port of the reference per-timestamp lift loop (temporal.py:33-53) at three sizes of the same
                 generator (N and delta scaled with m so E2/m stays that of the workload), fitted a*T*m + b*E2, EXTRAPOLATED to the
                 full workload (labelled as such; a direct run would take days);
      B-sorted : vectorised CPU lift (sort + searchsorted + repeat_interleave, identical output; not in the reference), FULL size;
      B-line   : lift_order_edge_index port (degree / cumsum / repeat_interleave) on the full-size event graph;
      B-agg    : aggregate_edge_index port (torch.unique(dim=0) + stable sort + scatter-add) for layers 1+2 at `--cpu-sample-events`;
      B-dbgnn  : pure-torch DBGNN train step (index_add_ message passing = what PyG dispatches on CPU) on that sample.
    `value` = lifted k-edges/s of the reference algorithm end to end (loop lift + aggregation + 1 DBGNN train step) on the largest
    B-loop sample."""
    import numpy as np
    from oracle import dbgnn as od
    from oracle import lift as ol
    from oracle import model as om
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # torch's intra-op pool: all host cores up to 64 (beyond that the fork/join of the many small ops of the reference loop costs more
    # than it gains: measured on the 256-thread GPU host, m = 32000: > 6 min with 256 threads against seconds with the ops kept serial)
    cores = max(min(avail, 64), 1)
    torch.set_num_threads(cores)
    cpu = torch.device("cpu")
    t_start = time.perf_counter()

    def note(msg):
        print(f"[cpu_baseline {time.perf_counter() - t_start:7.1f}s] {msg}", file=sys.stderr, flush=True)

    def sample(m, s):
        scale = m / args.events
        n = max(int(args.nodes * scale), 16)
        ei, t = synth_stream(m, n, args.span, s, cpu)              # same span and delta: E2/m = m*delta/(n*span) is preserved
        ei, t, _ = om.stable_time_sort(ei, t)
        return ei, t, n

    def train_step(layers, n, s):
        g = torch.Generator().manual_seed(s)
        data = om.dbgnn_inputs(layers, 2, "last", x=torch.randn(n, args.features, generator=g),
                               x_h=torch.randn(layers[2]["num_nodes"], args.features, generator=g))
        y = torch.randint(0, args.classes, (n,), generator=g)
        params = {k: v.requires_grad_(True) for k, v in od.init_params(args.classes, (args.features, args.features),
                                                                       [args.features] * 3, seed=s).items()}
        opt = torch.optim.Adam(params.values(), lr=1e-3)
        t0 = time.perf_counter()
        opt.zero_grad()
        torch.nn.functional.cross_entropy(od.forward(params, data), y).backward()
        opt.step()
        return time.perf_counter() - t0

    # ---- B-loop at three sizes
    loop = []
    m0 = min(args.cpu_loop_events, args.events)
    for k, m in enumerate((m0, 2 * m0, 4 * m0)):
        m = min(m, args.events)
        ei, t, n = sample(m, seed + k)
        t0 = time.perf_counter()
        ho = ol.temporal_lift_per_timestamp(ei, t, args.delta)
        dt = time.perf_counter() - t0
        loop.append({"m": m, "N": n, "T": int(torch.unique(t).numel()), "E2": int(ho.size(1)), "seconds": dt})
        note(f"B-loop m={m}: {dt:.2f}s")
        if dt * 8.0 > 60.0:                                  # the next size costs ~4-8x: stay inside the time budget
            break
    if len(loop) < 2:
        loop.append(dict(loop[0]))                            # degenerate fit (one size only): slope through that point
    a_mat = np.array([[r["T"] * r["m"], r["E2"]] for r in loop], dtype=np.float64)
    b_vec = np.array([r["seconds"] for r in loop], dtype=np.float64)
    coef, *_ = np.linalg.lstsq(a_mat, b_vec, rcond=None)
    coef = np.maximum(coef, 0.0)
    # largest loop sample: the rest of the reference step on it (aggregation + train step)
    big = loop[-1]
    ei, t, n = sample(big["m"], seed + len(loop) - 1)
    t0 = time.perf_counter()
    layers = om.layers_from_temporal(ei, t, n, delta=args.delta, max_order=2, loop_lift=True)
    t_layers = time.perf_counter() - t0
    t_train = train_step(layers, n, seed)
    note(f"reference step on the largest loop sample: layers {t_layers:.2f}s, train {t_train:.2f}s")
    # ---- B-sorted and B-line at FULL size
    ei_f, t_f = synth_stream(args.events, args.nodes, args.span, seed + 10, cpu)
    ei_f, t_f, _ = om.stable_time_sort(ei_f, t_f)
    t0 = time.perf_counter()
    ho_f = ol.temporal_lift_sorted(ei_f, t_f, args.delta, args.nodes)
    t_sorted = time.perf_counter() - t0
    e2_full = int(ho_f.size(1))
    t_total_full = float(coef[0] * torch.unique(t_f).numel() * args.events + coef[1] * e2_full)
    t0 = time.perf_counter()
    e3 = int(ol.line_graph_lift(ho_f, args.events).size(1))
    t_line = time.perf_counter() - t0
    note(f"B-sorted {t_sorted:.2f}s, B-line {t_line:.2f}s (full size)")
    del ho_f, ei_f, t_f
    # ---- B-agg + B-dbgnn on the vectorised pipeline sample
    ms = min(args.cpu_sample_events, args.events)
    ei_s, t_s, n_s = sample(ms, seed + 20)
    t0 = time.perf_counter()
    ho_s = ol.temporal_lift_sorted(ei_s, t_s, args.delta, n_s)
    t_lift_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    layers_s = om.layers_from_temporal(ei_s, t_s, n_s, delta=args.delta, max_order=2, event_graph=ho_s)
    t_agg_s = time.perf_counter() - t0
    note(f"B-agg {t_agg_s:.2f}s (m={ms})")
    t_train_s = train_step(layers_s, n_s, seed + 1)
    note(f"B-dbgnn {t_train_s:.2f}s")
    e2_s = int(ho_s.size(1))
    return {
        "value": big["E2"] / (t_layers + t_train),
        "unit": "lifted k-edges/s",
        "cores": cores,
        "host_threads_available": avail,
        "kind": "port",
        "sample": f"oracle port of the reference algorithm (per-timestamp lift loop + aggregation + 1 DBGNN train step) on m={big['m']} events, "
                  f"N={big['N']}, delta={args.delta}, E2={big['E2']}: lift+aggregate {t_layers:.2f}s, train step {t_train:.2f}s",
        "b_loop": {"samples": loop, "model": "seconds = a*T*m + b*E2", "a": float(coef[0]), "b": float(coef[1]),
                   "extrapolated_full_size_seconds": t_total_full,
                   "extrapolated_full_size_k_edges_per_s": e2_full / t_total_full if t_total_full > 0 else None,
                   "note": "EXTRAPOLATED from the three measured sizes to the full workload; not measured"},
        "b_sorted": {"m": args.events, "E2": e2_full, "seconds": t_sorted, "k_edges_per_s": e2_full / t_sorted,
                     "note": "vectorised CPU lift only (sort+searchsorted; not in the reference), FULL size"},
        "b_line": {"E2": e2_full, "E3": e3, "seconds": t_line, "out_edges_per_s": e3 / t_line, "note": "lift_order_edge_index port, FULL size"},
        "b_agg": {"m": ms, "N": n_s, "E2": e2_s, "seconds": t_agg_s,
                  "note": "layers 1+2 via the aggregate_edge_index port (torch.unique(dim=0) + stable sort + scatter-add) of a precomputed "
                          f"event graph (its vectorised lift took {t_lift_s:.2f}s)"},
        "b_dbgnn": {"m": ms, "N": n_s, "U2": layers_s[2]["num_nodes"], "F": args.features, "seconds": t_train_s, "steps_per_s": 1.0 / t_train_s},
        "vectorised_step_k_edges_per_s": e2_s / (t_lift_s + t_agg_s + t_train_s),
    }


# ---------------------------------------------------------------------------------------------------------------------------------
def hub_streams(dev) -> dict:
    """Graph construction (both layers + both GCN plans + the bipartite grouping) on two streams WITH hub nodes, fused order-2 builder against the
    generic kernels (lift -> coalesce -> coalesce -> plans), same stream, same box; `plans_identical`: every CSR array of both plans compared;
    `chosen_*`: the builder the callers take (`_hip.debruijn2_wanted`: the generic kernels from 2048 events per node on average)."""
    import pathpyg_amd as pp
    from pathpyg_amd import _hip
    from pathpyg_amd import distributed as ppd

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, out

    gen = torch.Generator(device=dev).manual_seed(3)
    report = {}
    for name, n, m, span, delta, scale_free in (("configs[2] generator: scale-free destinations, 1e6 nodes / 2e7 events", 1_000_000, 20_000_000, 10_000_000, 1_500_000, True),
                                                 ("contact stream: 96 nodes / 2e6 events", 96, 2_000_000, 2_000_000, 300, False)):
        src = torch.randint(0, n, (m,), generator=gen, device=dev)
        if scale_free:
            dst = (n * torch.rand(m, generator=gen, device=dev, dtype=torch.float64).pow(6.0)).long().clamp_(max=n - 1)
        else:
            dst = torch.randint(0, n, (m,), generator=gen, device=dev)
        t = torch.randint(0, span, (m,), generator=gen, device=dev)
        tg = pp.TemporalGraph(pp.Data(edge_index=torch.stack((src, dst)), time=t, num_nodes=n))
        del src, dst, t
        ms_f, built = timed(lambda: _hip.debruijn2(tg.data.edge_index, tg.data.time, n, delta, None), 3)
        ppd.FUSED_BUILDER = False
        x0 = torch.zeros(n, 4, device=dev)
        ms_g, shard = timed(lambda: ppd.build_dbgnn_shard(tg, delta, x0, lambda num_ho_nodes: torch.zeros(num_ho_nodes, 4, device=dev), None, ppd.Comm()).resolve(), 2)
        ppd.FUSED_BUILDER = True
        same = built is not None and all(torch.equal(getattr(built.ho, f), getattr(shard.ho.plan, f)) and torch.equal(getattr(built.fo, f), getattr(shard.fo.plan, f))
                                         for f in ("fwd_ptr", "fwd_idx", "fwd_val", "bwd_ptr", "bwd_idx", "bwd_val", "self_coef"))
        chosen = "fused" if (built is not None and _hip.debruijn2_wanted(m, n)) else "generic"
        report[name] = {"delta": delta, "fused_builder_ms": ms_f, "generic_kernels_ms": ms_g, "builder": "fused" if built is not None else "generic (fallback)",
                        "chosen_by_from_temporal_graph_and_build_dbgnn_shard": chosen, "chosen_ms": ms_f if chosen == "fused" else ms_g,
                        "plans_identical": bool(same), **({k: built.sizes[k] for k in ("E2", "U2", "A2", "hub_nodes", "hub_tasks")} if built is not None else {})}
        del built, shard, tg, x0
        torch.cuda.empty_cache()
    return report


def multi_order(g, nodes: int, delta, dev) -> dict:
    """The multi-order half of the metric (BASELINE configs[2] "k = 1..3 lift only", configs[4] "k = 2..5 lift"): untimed for `value`.
    ``MultiOrderModel.from_temporal_graph(g, delta, K)`` for K = 2..5 on the headline stream and K = 1..3 on the configs[2] generator — wall time
    per call, and per LAYER (HIP events around the C calls of the level-by-level builder, pp_multiorder_prepare / pp_multiorder_step): instance
    edges E_k the reference lifts, nodes U_k, edges A_k, the SURVEY §8(d) bytes of the generic pipeline for that layer (line-graph lift
    16 E_{k-1} + 16 E_k, coalesce 20 E_k + 20 A_k; layer 2: the temporal lift's 24 m + 16 E_2) and the bytes this builder moves
    (16 I_{k-1} + 48 I_k + 20 A_k: parent records in, child records out and in again, the window table read per child, the layer and the next
    level's type arrays out; top layer: 16 I_{k-1} + 24 I_k + 8 A_k — 4-byte child records, columns + weights only),
    both over the layer's time against 8 TB/s."""
    import pathpyg_amd as pp
    from pathpyg_amd import _hip

    def wall(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, out

    def per_layer(tg, n, d, k_max):
        data = tg.data
        best = None
        for _ in range(3):
            clock = []
            built = _hip.multi_order_temporal(data.edge_index, data.time, n, d, None, k_max, clock=clock)
            torch.cuda.synchronize()
            if built is None:
                return None
            ms = [a.elapsed_time(b) for _, a, b in clock]
            if best is None or sum(ms) < sum(best):
                best = ms
        m_events = built[0].n_instances
        rows = [{"phase": "continuation windows + layer 1 (pp_temporal_count + pp_multiorder_prepare)", "ms": best[0], "U": built[0].n_nodes,
                 "A": built[0].n_edges, "E": m_events}]
        for k in range(2, k_max + 1):
            b, prev = built[k - 1], built[k - 2]
            table = (24 * m_events + 16 * b.n_instances if k == 2 else 16 * prev.n_instances + 16 * b.n_instances) + 20 * b.n_instances + 20 * b.n_edges
            top = k == k_max          # (the top layer's children are 4-byte records and only columns + weights come out)
            moved = 16 * prev.n_instances + (24 if top else 48) * b.n_instances + (8 if top else 20) * b.n_edges
            ms_k = best[k - 1]
            rows.append({"phase": f"layer {k} (pp_multiorder_step)", "ms": ms_k, "U": b.n_nodes, "A": b.n_edges, "E": b.n_instances,
                         "table_bytes": table, "moved_bytes": moved,
                         "frac_table": table / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS, "frac_moved": moved / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS})
        del built
        return rows

    report = {"what": "MultiOrderModel.from_temporal_graph(g, delta, max_order = K): wall ms per call, then the layers one by one (HIP events); outside the timed "
                      "region; E = instance edges of the reference's lift, U / A = nodes / edges of the layer; fractions of 8 TB/s",
              "builder": "level by level (pp_multiorder_prepare / pp_multiorder_step) from K = 3 on, fused order-2 builder (pp_debruijn2_*) at K = 2"}
    head = {}
    for k in (2, 3, 4, 5):
        ms, mom = wall(lambda: pp.MultiOrderModel.from_temporal_graph(g, delta=delta, max_order=k))
        head[f"K={k}"] = {"ms": ms, "level_by_level": "layers" in getattr(mom, "sizes", {})}
        del mom
    head["layers"] = per_layer(g, nodes, delta, 5)
    report["headline stream"] = head
    torch.cuda.empty_cache()
    gen = torch.Generator(device=dev).manual_seed(3)
    n, m, span, d2 = 1_000_000, 20_000_000, 10_000_000, 1_500_000
    src = torch.randint(0, n, (m,), generator=gen, device=dev)
    dst = (n * torch.rand(m, generator=gen, device=dev, dtype=torch.float64).pow(6.0)).long().clamp_(max=n - 1)
    t = torch.randint(0, span, (m,), generator=gen, device=dev)
    tg = pp.TemporalGraph(pp.Data(edge_index=torch.stack((src, dst)), time=t, num_nodes=n))
    del src, dst, t
    c2 = {"delta": d2}
    for k in (1, 2, 3):
        ms, mom = wall(lambda: pp.MultiOrderModel.from_temporal_graph(tg, delta=d2, max_order=k))
        c2[f"K={k}"] = {"ms": ms, "level_by_level": "layers" in getattr(mom, "sizes", {})}
        del mom
    c2["layers"] = per_layer(tg, n, d2, 3)
    report["configs[2] generator: scale-free destinations, 1e6 nodes / 2e7 events"] = c2
    del tg
    torch.cuda.empty_cache()
    # BASELINE configs[4]'s lift ("100M-edge temporal stream, multi-order k = 2..5 lift") on ONE GPU: 10^8 events / 5 * 10^6 nodes, delta tuned so that
    # E_k ~ m at every order (the stream of tests/test_gpu_scale.py::test_config4_100m_events_k2_to_k5_lift_properties)
    n, m, span, d4 = 5_000_000, 100_000_000, 100_000_000, 5_000_000
    gen = torch.Generator(device=dev).manual_seed(7)
    src = torch.randint(0, n, (m,), generator=gen, device=dev)
    dst = torch.randint(0, n, (m,), generator=gen, device=dev)
    t = torch.randint(0, span, (m,), generator=gen, device=dev)
    tg = pp.TemporalGraph(pp.Data(edge_index=torch.stack((src, dst)), time=t, num_nodes=n))
    del src, dst, t
    c4 = {"delta": d4}
    torch.cuda.reset_peak_memory_stats(dev)
    ms, mom = wall(lambda: pp.MultiOrderModel.from_temporal_graph(tg, delta=d4, max_order=5), reps=2)
    c4["K=5"] = {"ms": ms, "level_by_level": "layers" in getattr(mom, "sizes", {}), "peak_hbm_gib": torch.cuda.max_memory_allocated(dev) / 2 ** 30}
    del mom
    c4["layers"] = per_layer(tg, n, d4, 5)
    report["configs[4] stream: 1e8 events / 5e6 nodes, one GPU"] = c4
    del tg
    torch.cuda.empty_cache()
    return report


def relaunch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under torch.distributed.run on this node."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


# ---- xGMI link model of the projection (bench.py --emulate-ranks): every pair of the 8 GPUs of a node has its own link; "7 links x ~153 GB/s
# per GPU" is the bidirectional figure, i.e. 76.8 GB/s per direction and link.  A collective is priced at its busiest link.
XGMI_GBS_PER_DIRECTION = 76.8
XGMI_EFFICIENCY = 0.8            # share of the link rate a large RCCL transfer sustains (assumption, stated in the report)
COLLECTIVE_LATENCY_US = 15.0     # launch + synchronisation cost of one collective (assumption)


def price_collectives(events, steps: int) -> dict:
    """Per-step cost of the logged collectives of ONE rank on the link model above: each costs latency + bytes-on-its-busiest-link / rate;
    `overlapped` ones were issued asynchronously with independent kernels queued behind them (pathpyg_amd.nn.sharded._ShardedTrunk)."""
    rate = XGMI_GBS_PER_DIRECTION * XGMI_EFFICIENCY * 1e9
    out = {"exposed_ms": 0.0, "overlapped_ms": 0.0, "collectives_per_step": len(events) / max(steps, 1), "by_kind": {}}
    for kind, nbytes, overlapped in events:
        ms = (COLLECTIVE_LATENCY_US * 1e-6 + nbytes / rate) * 1e3 / max(steps, 1)
        out["overlapped_ms" if overlapped else "exposed_ms"] += ms
        k = out["by_kind"].setdefault(kind + (" (async)" if overlapped else ""), {"count_per_step": 0.0, "busiest_link_bytes_per_step": 0.0, "ms_per_step": 0.0})
        k["count_per_step"] += 1.0 / max(steps, 1)
        k["busiest_link_bytes_per_step"] += nbytes / max(steps, 1)
        k["ms_per_step"] += ms
    return out


def simulate_async(events, windows, steps: int, timeline: list | None = None) -> float:
    """Per-step time ONE rank would still wait for its asynchronous collectives: every such collective was logged with the positions of its
    issue and of its wait on the rank's compute clock (`Comm.windows`).  One queue for the rank's links (each of these collectives loads all
    seven): a transfer starts when it is issued and the previous one has finished, takes latency + bytes-on-the-busiest-link / rate, and the
    rank stalls at the wait for whatever is not finished by then (stalls push everything behind them)."""
    rate = XGMI_GBS_PER_DIRECTION * XGMI_EFFICIENCY * 1e9
    items = []
    for idx, p_issue, p_wait in windows:
        items.append((p_issue, 0, idx))
        items.append((max(p_wait, p_issue), 1, idx))
    items.sort()
    link_free, stall, finish, cost, issued = 0.0, 0.0, {}, {}, {}
    for pos, kind, idx in items:
        now = pos + stall
        if kind == 0:
            start = max(now, link_free)
            cost[idx] = (COLLECTIVE_LATENCY_US * 1e-6 + events[idx][1] / rate) * 1e3
            issued[idx] = pos
            finish[idx] = start + cost[idx]
            link_free = finish[idx]
        else:
            late = max(finish.get(idx, 0.0) - now, 0.0)
            stall += late
            if timeline is not None:
                timeline.append({"kind": events[idx][0], "MB_on_busiest_link": round(events[idx][1] / 1e6, 2), "issued_at_ms": round(issued[idx], 3),
                                 "waited_at_ms": round(pos, 3), "link_ms": round(cost[idx], 3), "stall_ms": round(late, 3)})
    return stall / max(steps, 1)


def cpu_baseline_isolated(args) -> dict:
    """The CPU baseline in its own process (no HIP runtime threads beside the host cores it measures) and under a hard time limit."""
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only"]
    for k in ("events", "nodes", "span", "delta", "features", "classes", "cpu_loop_events", "cpu_sample_events"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.cpu_baseline_timeout)
    except subprocess.TimeoutExpired as exc:
        tail = (exc.stderr or b"")[-400:]
        return {"value": None, "unit": "lifted k-edges/s", "cores": None, "kind": "port",
                "sample": f"CPU baseline exceeded its {args.cpu_baseline_timeout}s limit and was stopped", "progress": tail.decode(errors="replace") if isinstance(tail, bytes) else str(tail)}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"value": None, "unit": "lifted k-edges/s", "cores": None, "kind": "port", "sample": "CPU baseline failed: " + r.stderr[-400:]}
    return json.loads(lines[-1])


def emulate(args) -> int:
    """`--emulate-ranks R`: the R ranks of the partition step as R THREADS on cuda:0 (pathpyg_amd.distributed.ThreadWorld): they take
    turns, so a rank's turns add up to the compute time it would need on a GPU of its own (kernels + launches + its read-backs; the copies
    that stand in for the collectives are not counted); every collective is logged with the bytes on its busiest link and priced on the
    xGMI link model.  Prints a PROJECTION of the R-GPU step, labelled as such — not a measurement of R GPUs."""
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: pathpyg_amd has no CPU path")
    import pathpyg_amd as pp
    from pathpyg_amd import distributed as ppd
    world = args.emulate_ranks
    if args.emulate_clock == "events":
        # host waits (a read-back behind the other ranks' queued kernels) must SLEEP, not spin: the host side of a rank is priced by its thread's CPU time
        import ctypes
        try:
            rc = ctypes.CDLL("libamdhip64.so").hipSetDeviceFlags(ctypes.c_uint(4))          # hipDeviceScheduleBlockingSync
            if rc != 0:
                print(f"bench.py: hipSetDeviceFlags(blocking sync) -> {rc}", file=sys.stderr)
        except OSError as exc:
            print(f"bench.py: hipSetDeviceFlags not available ({exc})", file=sys.stderr)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ei, t = synth_stream(args.events, args.nodes, args.span, seed=1, device=dev)
    g = pp.TemporalGraph(pp.Data(edge_index=ei, time=t, num_nodes=args.nodes))
    del ei, t
    n_ho = int(pp.MultiOrderModel.from_temporal_graph(g, delta=1, max_order=1).layers[1].m)
    feat = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(args.nodes, args.features, generator=feat, device=dev)          # resident inputs, shared by the emulated ranks
    x_h = torch.randn(n_ho, args.features, generator=feat, device=dev)
    y = torch.randint(0, args.classes, (args.nodes,), generator=feat, device=dev)
    # features through resident row stores (a rank's owned rows stay placed, its halo rows are fetched per step); the label vector (8 bytes per
    # node) is handed over whole: a rank's labels are then a VIEW of it, and the class-range check of the loss is remembered on the base tensor
    loaders = (ResidentRows(x), ResidentRows(x_h), y)

    # identical initial weights on every rank, as in the multi-process run — drawn ONCE here: the emulated ranks are threads that share torch's
    # global generator, seeding it in every thread would race (each rank would start from different weights)
    torch.manual_seed(0)
    init_state = pp.nn.DBGNN(num_classes=args.classes, num_features=(args.features, args.features), hidden_dims=[args.features] * 3,
                             p_dropout=args.dropout).to(dev).state_dict()

    alloc_mark = {}

    def body(comm):
        net = pp.nn.DBGNN(num_classes=args.classes, num_features=(args.features, args.features), hidden_dims=[args.features] * 3,
                          p_dropout=args.dropout).to(dev)
        net.load_state_dict(init_state)
        opt = pp.nn.optim.Adam(net.parameters(), lr=1e-3)                            # (pp_adam_f32: one launch over all parameter tensors)
        sharded = ppd.ShardedDBGNN(net, comm, overlap=not args.no_overlap)
        if args.trace:
            comm.trace = {}
        build_laps, sizes, loss = [], {}, None
        prof = None
        for it in range(args.warmup + args.steps):
            if it == args.warmup:
                comm.end_turns()
                comm.tw.plain_barrier.wait()
                if comm.rank == 0:          # the ranks are threads of ONE interpreter: a cyclic-GC pass over everybody's garbage would be billed to
                    import gc               # whichever rank's turn it interrupts (a process per rank collects only its own) -> collect once, then off
                    gc.collect()
                    gc.disable()
                    alloc_mark["device_mallocs_before_timed"] = int(torch.cuda.memory_stats().get("num_device_alloc", 0))
                comm.tw.plain_barrier.wait()
                comm.reset_counters()
                if args.host_profile and comm.rank == min(1, world - 1):
                    import cProfile
                    prof = cProfile.Profile()
                    prof.enable()
            comm.barrier()                          # (step boundary: opens this rank's first turn of the step)
            opt.zero_grad(set_to_none=True)
            c0 = comm.lap()
            shard = ppd.build_dbgnn_shard(g, args.delta, *loaders, comm, defer_status=True)
            if it >= args.warmup:
                build_laps.append((c0, comm.lap()))
            loss = sharded.loss(shard)
            loss.backward()
            ppd.all_reduce_gradients(net, average=False, comm=comm, inplace_views=True)
            opt.step()
            comm.mark("step: gradient all-reduce + Adam")
            sizes = shard.sizes
        if prof is not None:
            prof.disable()
            import io
            import pstats
            buf = io.StringIO()
            st = pstats.Stats(prof, stream=buf)
            st.sort_stats("tottime").print_stats(70)
            st.sort_stats("cumtime").print_stats(r"pathpyg_amd|bench\.py|optim", 90)
            with open(args.host_profile, "w") as fh:
                fh.write(f"# cProfile of rank {comm.rank} of {world} emulated ranks over {args.steps} steps\n" + buf.getvalue())
        comm.end_turns()
        timed = {"compute_s": comm.compute_s, "host_s": comm.host_s, "build_s": sum(comm.between(a_, b_) for a_, b_ in build_laps),
                 "windows": [(i_, comm.position(a_) * 1e3, comm.position(b_) * 1e3) for i_, a_, b_ in comm.windows],
                 "events": list(comm.events), "sent": dict(comm.sent_bytes), "trace": dict(comm.resolve_trace() or {}) if comm.trace is not None else None}
        sizes = ppd.global_sizes(shard, comm)
        total = loss.detach().to(torch.float64).reshape(1).clone()
        comm.all_reduce_(total)
        return {**timed, "sizes": sizes, "loss": float(total)}

    results = ppd.run_thread_world(world, body, dev, clock=args.emulate_clock)
    import gc
    gc.enable()
    steps = args.steps
    device_ms = [r["compute_s"] * 1e3 / steps for r in results]
    host_ms = [r["host_s"] * 1e3 / steps for r in results]
    # "events" clock: a rank's turns cost what its queue cost (kernels + the waits for its own host inside a turn); a rank whose host needs longer
    # than that is host-bound on a GPU of its own too -> max(host, device).  "drain" clock: the drained wall time is both.
    compute_ms = [max(d_, h_) for d_, h_ in zip(device_ms, host_ms)] if args.emulate_clock == "events" else device_ms
    build_ms = [r["build_s"] * 1e3 / steps for r in results]
    # the rank with the costliest collectives sets the pace of every collective
    priced_all = [price_collectives(r["events"], steps) for r in results]
    priced = max(priced_all, key=lambda p_: p_["exposed_ms"] + p_["overlapped_ms"])
    slowest = max(compute_ms)
    dbgnn_ms = max(c - b for c, b in zip(compute_ms, build_ms))
    hidden = min(priced["overlapped_ms"], dbgnn_ms)
    # the asynchronous collectives against the compute that actually ran between their issue and their wait, rank by rank
    stall_ms = [simulate_async(r["events"], r["windows"], steps) for r in results]
    timeline = []
    simulate_async(results[min(1, world - 1)]["events"], results[min(1, world - 1)]["windows"], steps, timeline)
    per_step = max(len(timeline) // max(steps, 1), 1)
    exposed_ms = [p_["exposed_ms"] for p_ in priced_all]
    step_ms = [c + e + s_ for c, e, s_ in zip(compute_ms, exposed_ms, stall_ms)]
    sz = results[0]["sizes"]
    report = {
        "what": f"PROJECTION of the {world}-GPU partition step from {world} ranks taking turns on ONE MI355X (threads of one process; NOT a measurement of "
                f"{world} GPUs)",
        "emulated_ranks": world, "steps": steps, "warmup": args.warmup, "overlap_schedule": not args.no_overlap,
        "clock": ("events: every turn of a rank bracketed by two stream events, nothing drained at the collectives (a stream-ordered RCCL run blocks its host only at the "
                  "size read-back); per rank max(device time of its turns, CPU time of its thread in its turns)" if args.emulate_clock == "events" else
                  "drain: the GPU is drained at the end of every turn (~45 per step) and the turn's wall time counts — an upper bound"),
        "per_rank_device_ms": device_ms, "per_rank_host_ms": host_ms,
        "workload": f"m={args.events}, N={args.nodes}, span={args.span}, delta={args.delta}, F={args.features}",
        "per_rank_compute_ms": compute_ms, "per_rank_graph_build_ms": build_ms,
        "max_rank_compute_ms": slowest, "mean_rank_compute_ms": sum(compute_ms) / world, "median_rank_compute_ms": sorted(compute_ms)[world // 2],
        # (all emulated ranks share ONE caching allocator: a retry = a failed hipMalloc answered by freeing the cache, paid by whichever rank's turn it hits)
        "emulation_allocator": {"peak_allocated_gib": torch.cuda.max_memory_allocated() / 2 ** 30, "peak_reserved_gib": torch.cuda.max_memory_reserved() / 2 ** 30,
                                "alloc_retries": int(torch.cuda.memory_stats().get("num_alloc_retries", 0)),
                                "device_mallocs": int(torch.cuda.memory_stats().get("num_device_alloc", 0)),
                                "device_mallocs_in_timed_steps": int(torch.cuda.memory_stats().get("num_device_alloc", 0)) - alloc_mark.get("device_mallocs_before_timed", 0)},
        "per_rank": {k: [r["sizes"].get(k) for r in results] for k in ("E2_local", "A2_local", "lift_events_local", "layer1_events_local", "ho_halo", "fo_halo")},
        "collectives_costliest_rank": priced,
        "link_model": {"GB_per_s_per_direction_and_link": XGMI_GBS_PER_DIRECTION, "efficiency": XGMI_EFFICIENCY,
                       "latency_us_per_collective": COLLECTIVE_LATENCY_US,
                       "note": "every GPU pair of a node has its own xGMI link; a collective costs latency + bytes on its busiest link / rate"},
        "comm_bytes_per_step_rank0": {k: v / steps for k, v in results[0]["sent"].items()},
        "projected_ms_per_step_no_overlap": slowest + priced["exposed_ms"] + priced["overlapped_ms"],
        "projected_ms_per_step": max(step_ms),
        "projected_ms_per_step_aggregate_model": slowest + priced["exposed_ms"] + priced["overlapped_ms"] - hidden,
        "per_rank_async_stall_ms": stall_ms,
        "async_timeline_rank1_last_step": [dict(e_, issued_at_ms=round(e_["issued_at_ms"] - timeline[-per_step]["issued_at_ms"], 3),
                                                waited_at_ms=round(e_["waited_at_ms"] - timeline[-per_step]["issued_at_ms"], 3)) for e_ in timeline[-per_step:]],
        "amdahl_terms_ms": {"slowest_rank_compute": slowest, "of_which_graph_build": max(build_ms), "collectives_exposed": priced["exposed_ms"],
                            "collectives_async": priced["overlapped_ms"], "async_still_in_flight_at_its_wait": max(stall_ms),
                            "async_hidden_behind_dbgnn_kernels": hidden,
                            "note": "projected = max over ranks of compute + blocking collectives + what its asynchronous collectives still have in flight at "
                                    "their waits (simulate_async: issue / wait positions on the rank's compute clock, one queue for its links); the "
                                    "aggregate model (round 3: sum of asynchronous link time against the DBGNN kernels' time) is kept beside it"},
        "loss": results[0]["loss"], "E2": sz.get("E2"), "U2": sz.get("U2"), "A2": sz.get("A2"),
    }
    if args.trace:
        report["phase_ms_rank1"] = {k: v * 1e3 / steps for k, v in (results[min(1, world - 1)]["trace"] or {}).items()}
        report["phase_ms_rank0"] = {k: v * 1e3 / steps for k, v in (results[0]["trace"] or {}).items()}
        report["phase_ms_last_rank"] = {k: v * 1e3 / steps for k, v in (results[world - 1]["trace"] or {}).items()}
    print(json.dumps(report), flush=True)
    return 0


DUMP_SAMPLE = 1 << 18          # entries kept of a larger array (float64: 2 MB each)
DUMP_LIMIT = 64 << 20


def dump_outputs(out_dir: str, loss, net, shard) -> None:
    """`--dump-outputs`: what the last timed step handed its caller — the loss, the weights after the optimiser step and their gradients —
    and the graph it built (first- and order-2 GCN plans of `shard`, partition path).  Integer arrays as float64 (exact below 2^53); an
    array of more than DUMP_SAMPLE entries is replaced by the entries at DUMP_SAMPLE indices drawn with a fixed seed (`<name>.sample_idx`)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss.detach().to(torch.float64).reshape(1)}
    for name, p in net.named_parameters():
        arrays[f"param.{name}"] = p.detach().float()
        if p.grad is not None:
            arrays[f"grad.{name}"] = p.grad.detach().float()
    if shard is not None:
        for layer, plan in (("fo", shard.fo.plan), ("ho", shard.ho.plan)):
            n_dst = int(plan.n_dst)
            ptr = plan.fwd_ptr[: n_dst + 1]
            nnz = int(ptr[-1])
            arrays[f"plan_{layer}.fwd_ptr"] = ptr
            arrays[f"plan_{layer}.fwd_idx"] = plan.fwd_idx[:nnz]
            if plan.fwd_val is not None:
                arrays[f"plan_{layer}.fwd_val"] = plan.fwd_val[:nnz]
            if plan.self_coef is not None:
                arrays[f"plan_{layer}.self_coef"] = plan.self_coef[:n_dst]
    total = 0
    for name, t in arrays.items():
        t = t.detach().reshape(-1)
        if t.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(12345).integers(0, t.numel(), DUMP_SAMPLE))
            np.save(os.path.join(out_dir, f"{name}.sample_idx.npy"), idx.astype(np.float64))
            total += idx.size * 8
            t = t[torch.from_numpy(idx).to(t.device)]
        a = t.cpu().numpy()
        a = a.astype(np.float32 if a.dtype in (np.float32, np.float16) else np.float64)
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        total += a.nbytes
    assert total <= DUMP_LIMIT, f"--dump-outputs wrote {total} bytes (limit {DUMP_LIMIT})"


def main() -> int:
    args = parse()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(args, seed=11)), flush=True)
        return 0
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ          # started by torch.distributed.run
    if args.halo_row_backward:
        import pathpyg_amd.nn.sharded as _sh
        _sh.OWNED_ROW_BACKWARD = False
    if args.builder == "generic":
        import pathpyg_amd.core.multi_order_model as _mm0
        import pathpyg_amd.distributed as _pd0
        _pd0.FUSED_BUILDER = False
        _mm0.FUSED_BUILDER = False
    if args.fo_halo != "auto":
        import pathpyg_amd.distributed as _pd
        _pd.FO_DENSE_HALO = args.fo_halo == "dense"
    if args.emulate_ranks > 1:
        return emulate(args)
    if args.gpus > 1 and not launched:
        return relaunch(args)
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if launched:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: pathpyg_amd has no CPU path")
    if not args.share_gpu and world > torch.cuda.device_count():
        raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} GPU(s) visible (use --share-gpu --backend gloo to test)")
    dev_index = 0 if args.share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    import torch.distributed as dist
    if launched:
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    import pathpyg_amd as pp
    from pathpyg_amd import distributed as ppd
    from pathpyg_amd._lib import lib

    mode_note = None
    if args.mode == "auto":
        args.mode = "partition" if (world == 1 or world >= 8) else "streams"
        if world > 1 and args.mode == "streams":
            mode_note = (f"{world} GPUs: the node-range partition of ONE stream is link-bound below 8 ranks on point-to-point xGMI (projected "
                         "42.7 ms at 2 ranks, 14.8 ms at 4 against 14.0 ms on one GPU) — this line runs independent streams (weak scaling, "
                         "weight-gradient all-reduce); `--mode partition` forces the split")
    partition = args.mode == "partition"
    if partition and world >= 8 and mode_note is None:
        # (say the bound in the line instead of leaving "≥ 6x at 8 GPUs" implied)
        mode_note = (f"{world} GPUs, node-range partition of ONE stream: on a locality-free (ER) stream every order-2 row crosses a link once per layer and "
                     "direction — ~3.1 ms of xGMI time per rank-step at fp32, F = 64 (76.8 GB/s x 0.8 per link pair + 15 us per exchange, a model that "
                     "was never calibrated on hardware) — beside a per-rank device time of 4.2-4.8 ms where 13.8 / 8 = 1.7 ms is ideal (197 launches "
                     "per rank-step): the projected 8-rank step is 6.0-6.5 ms = 2.1-2.3x of one GPU, and ~4.5x is the link-bound ceiling of this "
                     "workload at fp32; north_star's >= 6x is out of reach for it (DESIGN §6)")
    comm = ppd.Comm()
    # ---- inputs, resident in HBM before the timed region.  partition: ONE stream replicated on every rank; streams: one per rank
    ei, t = synth_stream(args.events, args.nodes, args.span, seed=1 + (0 if partition else rank), device=dev)
    # library load, first-launch costs and the sort workspace (allocator growth) are paid by an untimed pass over the same stream
    pp.TemporalGraph(pp.Data(edge_index=ei.clone(), time=t.clone(), num_nodes=args.nodes))
    sort0, sort1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sort0.record()
    g = pp.TemporalGraph(pp.Data(edge_index=ei, time=t, num_nodes=args.nodes))       # a1: stable time sort (HIP radix sort) + permutation
    sort1.record()
    del ei, t
    n_ho = int(pp.MultiOrderModel.from_temporal_graph(g, delta=1, max_order=1).layers[1].m)      # order-2 nodes = distinct (src, dst) pairs
    feat = torch.Generator(device=dev).manual_seed(7 + (0 if partition else rank))
    x = torch.randn(args.nodes, args.features, generator=feat, device=dev)
    x_h = torch.randn(n_ho, args.features, generator=feat, device=dev)
    y = torch.randint(0, args.classes, (args.nodes,), generator=feat, device=dev)
    torch.manual_seed(0)                                    # identical initial weights on every rank
    net = pp.nn.DBGNN(num_classes=args.classes, num_features=(args.features, args.features),
                      hidden_dims=[args.features] * 3, p_dropout=args.dropout).to(dev)
    opt = pp.nn.optim.Adam(net.parameters(), lr=1e-3)                               # (pp_adam_f32: one launch over all parameter tensors)
    sharded = ppd.ShardedDBGNN(net, comm, overlap=not args.no_overlap) if partition else None
    # world size > 1: a rank reads only its owned + halo rows of the (resident) inputs
    x_in, xh_in, y_in = (x, x_h, y) if world == 1 else (ResidentRows(x), ResidentRows(x_h), y)      # owned rows resident, halo rows fetched per step
    lift_ms = []
    sizes = {}

    def step_partition(timed: bool):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        opt.zero_grad(set_to_none=True)
        e0.record()
        shard = ppd.build_dbgnn_shard(g, args.delta, x_in, xh_in, y_in, comm, defer_status=True)
        e1.record()
        if timed:                                   # (bookkeeping of the live rooflines: pointers -> CSR sizes)
            for gs in (shard.fo, shard.ho):
                register_plan(gs.plan)
            register_plan(shard.bip)
            SRC_ROWS[shard.bip.fwd_idx.data_ptr()] = shard.ho.n_own
            SRC_ROWS[shard.bip.bwd_idx.data_ptr()] = shard.bip.n_dst
        loss = sharded.loss(shard)
        loss.backward()
        ppd.all_reduce_gradients(net, average=False, comm=comm, inplace_views=True)
        opt.step()
        sizes.update(shard.sizes)
        step_partition.last_shard = shard
        if timed:
            lift_ms.append((e0, e1))
        return loss

    def step_streams(timed: bool):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mom = pp.MultiOrderModel.from_temporal_graph(g, delta=args.delta, max_order=2)
        data = mom.to_dbgnn_data(max_order=2, mapping="last", x=x, x_h=x_h)
        e1.record()
        opt.zero_grad(set_to_none=True)
        loss = pp.nn.cross_entropy(net(data), y)
        loss.backward()
        if launched:        # data-parallel over independent streams: only the ~20 k weight gradients cross xGMI (one all-reduce)
            ppd.all_reduce_gradients(net)
        opt.step()
        if timed:
            lift_ms.append((e0, e1))
        if "E2" not in sizes:
            sizes.update({"m": args.events, "N": args.nodes, "E2": int(pp.algorithms.lift_order_temporal(g, args.delta).size(1)),
                          "U2": mom.layers[2].n, "A1": mom.layers[1].m, "A2": mom.layers[2].m})
        return loss

    step = step_partition if partition else step_streams
    if not partition:        # the API path builds its plans inside DBGNN.forward: register their shapes as they are made
        from pathpyg_amd import _hip

        def registering(fn, src_rows=None):
            def wrapped(*a, **kw):
                plan = fn(*a, **kw)
                register_plan(plan)
                SRC_ROWS[plan.fwd_idx.data_ptr()], SRC_ROWS[plan.bwd_idx.data_ptr()] = plan.n_src, plan.n_dst
                return plan
            return wrapped
        _hip.gcn_plan, _hip.bipartite_plan = registering(_hip.gcn_plan), registering(_hip.bipartite_plan)
        _hip.bipartite_plan_from_edge_grouping = registering(_hip.bipartite_plan_from_edge_grouping)
        fused_api = _hip.debruijn2

        def debruijn2_registering(*a, **kw):          # the API path on the fused builder: its plans come out of pp_debruijn2_*
            built = fused_api(*a, **kw)
            if built is not None:
                for plan in (built.fo, built.ho):
                    register_plan(plan)
                    SRC_ROWS[plan.fwd_idx.data_ptr()], SRC_ROWS[plan.bwd_idx.data_ptr()] = plan.n_src, plan.n_dst
                sizes.update(built.sizes)
                sizes["builder"] = "fused"
            return built
        _hip.debruijn2 = debruijn2_registering

    def barrier():
        if launched:
            dist.barrier()
        torch.cuda.synchronize()

    L = lib()

    def lift_desc(ei_p, t_p, tdt, m, n_own, *rest):
        return ("temporal lift (pp_temporal_count .. pp_temporal_fill)", 24 * m)

    def coalesce_desc(ei_p, e, *rest):
        return (f"aggregation (pp_coalesce_count .. pp_coalesce_fill), {e:.2e} instance edges", 20 * e)

    with KernelClock(L, "pp_spmm_f32", spmm_desc) as spmm_clock, \
            KernelClock(L, "pp_gcn_forward_drop_f32", gcn_forward_desc) as fwd_clock, \
            KernelClock(L, "pp_gcn_backward_nnz_f32", gcn_backward_desc) as bwd_clock, \
            KernelClock(L, "pp_temporal_fill", lambda m, n, total, *r: ("k_expand (pp_temporal_fill)", 16 * total + 12 * m)) as fill_clock, \
            KernelClock(L, "pp_temporal_count", lift_desc, until="pp_temporal_fill") as lift_clock, \
            KernelClock(L, "pp_coalesce_count", coalesce_desc, until="pp_coalesce_fill") as agg_clock, \
            KernelClock(L, "pp_debruijn2_lists", lambda ei_p, t_p, tdt, m, *r: ("fused order-2 builder (pp_debruijn2_lists .. pp_debruijn2_fill)", 24 * m),
                        until=("pp_debruijn2_count", ("pp_debruijn2_fill_ready", "pp_debruijn2_fill"))) as fused_clock:
        clocks = (spmm_clock, fwd_clock, bwd_clock, fill_clock, lift_clock, agg_clock, fused_clock)
        for _ in range(args.warmup):
            step(False)
        barrier()
        comm.reset_counters()
        for c in clocks:
            c.enabled = True
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step(True)
        barrier()
        elapsed = time.perf_counter() - t0
        for c in clocks:
            c.enabled = False
        fused_ran = bool(fused_clock.records)
        if args.dump_outputs and rank == 0:            # (before anything else runs on the GPU: the buffers of the last timed step are intact)
            dump_outputs(args.dump_outputs, loss, net, getattr(step_partition, "last_shard", None) if partition else None)
        if fused_ran and rank == 0 and world == 1 and args.full:
            # the fused builder never writes the event graph: the lift / aggregation kernels it replaces (and the k_expand fill kernel the
            # north star's "40 % of HBM peak on the lift kernel" refers to) are timed here, OUTSIDE the timed region, on the same stream
            ppd.FUSED_BUILDER = False
            for c in (fill_clock, lift_clock, agg_clock):
                c.enabled = True
            for _ in range(3):
                generic = ppd.build_dbgnn_shard(g, args.delta, x_in, xh_in, y_in, comm)
            torch.cuda.synchronize()
            for c in (fill_clock, lift_clock, agg_clock):
                c.enabled = False
            ppd.FUSED_BUILDER = True
            generic_steps = 3
            del generic
        else:
            generic_steps = args.steps
    # The same step through the REFERENCE API (MultiOrderModel.from_temporal_graph -> to_dbgnn_data -> DBGNN.forward -> cross_entropy ->
    # backward -> Adam; reference multi_order_model.py:124-192, 511-554, nn/dbgnn.py:121-151), timed after the headline region on the same
    # stream and model: what a drop-in user of the reference API gets
    api_path = None
    if partition:
        sizes.update(ppd.global_sizes(step_partition.last_shard, comm))       # (A2 over all ranks: a collective, outside the timed region)
        step_partition.last_shard = None                                       # (the API steps below must not add this shard to the peak)
    peak_main = torch.cuda.max_memory_allocated(dev)
    if partition and rank == 0 and world == 1 and args.full and not args.no_api_path:
        torch.cuda.reset_peak_memory_stats(dev)
        api_sizes = dict(sizes)
        for _ in range(max(3, min(args.warmup, 5))):
            step_streams(False)
        torch.cuda.synchronize()
        ta = time.perf_counter()
        for _ in range(args.steps):
            step_streams(True)
        torch.cuda.synchronize()
        api_ms = 1e3 * (time.perf_counter() - ta) / args.steps
        api_lift = lift_ms[-args.steps:]
        del lift_ms[-args.steps:]
        api_path = {"what": "MultiOrderModel.from_temporal_graph(g, delta, max_order=2) -> to_dbgnn_data(x, x_h) -> DBGNN.forward -> cross_entropy -> "
                            "backward -> Adam, same stream / model / step count, timed after the headline region",
                    "ms_per_step": api_ms, "graph_construction_ms": sum(a.elapsed_time(b) for a, b in api_lift) / len(api_lift),
                    "builder": "fused (pp_debruijn2_*)" if getattr(pp.MultiOrderModel.from_temporal_graph(g, delta=args.delta, max_order=2), "_pp_fused", None)
                    is not None else "generic kernels"}
        api_path["peak_hbm_gib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        torch.cuda.reset_peak_memory_stats(dev)
        sizes.clear()
        sizes.update(api_sizes)
    # Streams with HUB NODES through the same builder (round 5; outside the timed region, rank 0 at one GPU): BASELINE configs[2]'s scale-free
    # generator and a contact stream of the shape of the reference's documented datasets — fused builder against the generic kernels, plans compared
    hub_report = None
    if partition and rank == 0 and world == 1 and args.full and not args.no_hub_streams:
        hub_report = hub_streams(dev)
    multi_order_report = None
    if partition and rank == 0 and world == 1 and args.full and not args.no_multi_order:
        multi_order_report = multi_order(g, args.nodes, args.delta, dev)
    # untimed extra: the k=2 -> k=3 line-graph lift of the same event graph (the lift kernel WITHOUT the continuation-list gather)
    k3 = None
    if rank == 0 and args.full:
        ho = pp.algorithms.lift_order_temporal(g, args.delta)
        with KernelClock(L, "pp_linegraph_fill", lambda e, n, total, *r: ("k_expand<no list> (pp_linegraph_fill)", 16 * total + 12 * e)) as lg_clock:
            lg_clock.enabled = True
            for _ in range(3):
                e3 = pp.algorithms.lift_order_edge_index(ho, num_nodes=args.events).size(1)
            torch.cuda.synchronize()
        (key, (n_lg, lg_ms, lg_b)), = lg_clock.groups().items()
        k3 = {"kernel": "k_tile_sources + " + key, "E3": e3, "launches": n_lg, "avg_launch_ms": lg_ms / max(n_lg, 1),
              "achieved": lg_b / (lg_ms * 1e-3) / 1e9 if lg_ms > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
              "frac": (lg_b / (lg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if lg_ms > 0 else 0.0}
        del ho
    e2_total = float(sizes.get("E2", 0))
    loss_total = loss.detach().to(torch.float64).reshape(1).clone()
    if launched and partition:
        comm.all_reduce_(loss_total)                             # every rank holds its share of the mean loss
    if launched:
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        comm.all_reduce_(tmax, dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        if not partition:                                        # streams: every rank lifted its own stream
            e2_all = torch.tensor([e2_total], device=dev, dtype=torch.float64)
            comm.all_reduce_(e2_all)
            e2_total = float(e2_all.item())

    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        lift = sum(a.elapsed_time(b) for a, b in lift_ms) / len(lift_ms)

        def entry(key, n_, ms_, b_, with_traffic=True, steps_=None):
            steps_ = args.steps if steps_ is None else steps_
            gbs = b_ / (ms_ * 1e-3) / 1e9 if ms_ > 0 else 0.0
            return {"kernel": key, "launches": n_, "avg_launch_ms": ms_ / max(n_, 1), "total_ms_per_step": ms_ / steps_, "achieved": gbs,
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                    "traffic": pmc_traffic(key, args) if (with_traffic and world == 1) else None,
                    # (`traffic` is NOT measured in this run: it is replayed from the committed rocprofv3 --pmc passes of this same command)
                    "traffic_source": pmc_traffic.source if (with_traffic and world == 1) else None,
                    "algorithmic_bytes_per_launch": b_ / max(n_, 1)}
        per_kernel = []
        for clock in (fwd_clock, bwd_clock, spmm_clock):
            for key, (n_, ms_, b_) in clock.groups().items():
                per_kernel.append(entry(key, n_, ms_, b_))
        per_kernel.sort(key=lambda r: -r["total_ms_per_step"])
        dominant = dict(per_kernel[0]) if per_kernel else None
        if dominant:
            dominant["bound"] = "hbm"
        (fill_key, (n_fill, fill_ms, fill_b)), = fill_clock.groups().items() if fill_clock.records else (("k_expand", (0, 0.0, 0)),)
        e2_rank = float(sizes.get("E2_local", sizes.get("E2", 0)))
        m_rank = float(sizes.get("m", args.events))
        lift_groups = lift_clock.groups()
        lift_total_ms = sum(v[1] for v in lift_groups.values())
        n_lift = sum(v[0] for v in lift_groups.values())
        lift_bytes = 24.0 * m_rank / max(world if partition else 1, 1) + 16.0 * e2_rank     # read (src,dst,t) of the shard, write [2,E2]
        lift_avg = lift_total_ms / max(n_lift, 1)
        agg_total_ms = sum(v[1] for v in agg_clock.groups().values()) / generic_steps
        a1, a2, u2 = float(sizes.get("A1", 0)), float(sizes.get("A2_local", sizes.get("A2", 0))), float(sizes.get("U2", 0))
        # 16 E_k + 4 E_k + 8 k U_k + 8 M_k + 20 A_k for layer 1 (instances = the m events, k = 1) and layer 2 (E2 pairs)
        agg_bytes = (20.0 * m_rank + 8.0 * args.nodes + 8.0 * m_rank + 20.0 * a1) + (20.0 * e2_rank + 16.0 * u2 + 8.0 * m_rank + 20.0 * a2)
        line = {
            "metric": "lifted k-edges/s (k=2 De Bruijn lift + aggregation + 1 DBGNN train step per pass, 10M temporal edges)",
            "value": e2_total * args.steps / elapsed,
            "unit": "lifted k-edges/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True,
            "scaling": "strong" if partition else "weak",
            **({"mode_note": mode_note} if mode_note else {}),
            "vs_baseline": None,
            "dtype": "int64 lift / f32 DBGNN",
            "data": "synthetic",
            "config": {"workload": f"temporal ER stream{'' if partition else ' per GPU'}: m={args.events} events, N={args.nodes} nodes, "
                                   f"t~U[0,{args.span}), delta={args.delta}, k=2, F={args.features}, hidden=[{args.features}]*3, classes={args.classes}"
                                   + (f", p_dropout={args.dropout}" if args.dropout else ""),
                       "parallelism": ((f"{world} rank(s) over {comm.backend or 'no process group'}: ONE global stream cut into node ranges — a rank builds the "
                                        "order-2 edges of its MIDDLE nodes from the events that touch them (no pair routing), destination-row DBGNN with one "
                                        "halo exchange per layer (all-to-all of contiguous row prefixes; first-order stack: all-gather), bipartite reduce-scatter, "
                                        "weight-gradient all-reduce") if world > 1 else "1 rank: the whole stream on one GPU (no collective)") if partition else
                                      ("1 GPU" if world == 1 else f"{world} independent streams, weight-gradient all-reduce (RCCL)"),
                       "graph_construction": ("fused node-by-node order-2 builder (pp_debruijn2_*): identical layers and plans, event graph not materialised"
                                              if sizes.get("builder") == "fused" else "generic kernels: lift -> coalesce -> plans"),
                       **{k: v for k, v in sizes.items() if not k.endswith("_cuts")}},
            "temporal_events_per_s": (1 if partition else world) * args.events * args.steps / elapsed,
            "time_sort_ms": sort0.elapsed_time(sort1),
            "lift_ms": lift,
            "lift_k_edges_per_s": sizes.get("E2", 0) / (lift * 1e-3),
            "dbgnn_step_ms": ms_step - lift,
            "dbgnn_steps_per_s": 1e3 / max(ms_step - lift, 1e-9),
            "loss": float(loss_total),
            "peak_hbm_gib": max(peak_main, torch.cuda.max_memory_allocated(dev)) / 2 ** 30,
            "comm_bytes_per_step_rank0": {k: v / args.steps for k, v in comm.sent_bytes.items()},
            "roofline": dominant,
            "kernel_rooflines": per_kernel,
            "lift_roofline": {"what": "whole temporal lift of this rank: count + scans + tail sort + fill (24 m_shard + 16 E2_shard bytes, SURVEY §8d)",
                              "avg_ms": lift_avg, "achieved": lift_bytes / (lift_avg * 1e-3) / 1e9 if lift_avg > 0 else 0.0, "peak": HBM_PEAK_GBS,
                              "unit": "GB/s", "frac": (lift_bytes / (lift_avg * 1e-3) / 1e9 / HBM_PEAK_GBS) if lift_avg > 0 else 0.0},
            "lift_fill_roofline": {**entry(fill_key, n_fill, fill_ms, fill_b, steps_=generic_steps),
                                   "north_star_claim": "north_star's '>= 40 % of HBM peak on the lift kernel' is measured on THIS kernel — k_expand, the fill of the "
                                                       "generic temporal lift that writes the [2, E2] event graph (its 16 E2 result bytes + 12 m source bytes over "
                                                       "its time) — in untimed passes; the timed step never writes the event graph (graph_build_roofline: the fused "
                                                       "order-2 builder, judged by its time), and from order 3 on the layers come from the level-by-level builder "
                                                       "(multi_order: per-layer times and byte counts)"},
            "generic_kernels_timed": ("inside the timed region" if not fused_ran else
                                      "lift_roofline / lift_fill_roofline / aggregation_roofline: 3 untimed passes of the generic kernels after the timed "
                                      "region (the timed steps build the graph with the fused order-2 builder, which never writes the event graph)"),
            "aggregation_roofline": {"what": "layers 1+2 of this rank: keys + radix sort + run heads + segment reduce (SURVEY §8d table bytes)",
                                     "ms_per_step": agg_total_ms, "achieved": agg_bytes / (agg_total_ms * 1e-3) / 1e9 if agg_total_ms > 0 else 0.0,
                                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                     "frac": (agg_bytes / (agg_total_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if agg_total_ms > 0 else 0.0},
            "linegraph_fill_roofline": k3,
        }
        if not args.full:           # (these need the untimed generic-kernel passes and the line-graph lift that only --full runs)
            for key in ("lift_roofline", "lift_fill_roofline", "generic_kernels_timed", "aggregation_roofline", "linegraph_fill_roofline"):
                del line[key]
        if api_path is not None:
            line["api_path_ms_per_step"] = api_path["ms_per_step"]
            line["api_path"] = api_path
        if hub_report is not None:
            line["hub_streams"] = hub_report
        if multi_order_report is not None:
            line["multi_order"] = multi_order_report
        if fused_ran:
            (fkey, (n_f, f_ms, _)), = fused_clock.groups().items()
            f_avg = f_ms / max(n_f, 1)
            # what the fused builder really moves per call (ADVICE r4 / VERDICT r4 #5): the events in (src, dst, t = 24 B each) and both
            # CSR plans out — first-order: 2 row-pointer arrays, (index, coefficient) both ways, self coefficients, the bipartite grouping;
            # order-2: the same over U2 rows / A2 edges (+ the merged weights when the API path keeps them).  The event graph [2, E2] is
            # never written, so the SURVEY §8d bytes of the generic pipeline are NOT bytes this builder moves: they are kept beside,
            # labelled, as an equivalent-work speed, and no fraction-of-peak claim rests on them.
            n_nodes = float(args.nodes)
            moved = (24.0 * m_rank + (8.0 * (n_nodes + 1) + 16.0 * a1 + 4.0 * n_nodes + 4.0 * a1)
                     + (8.0 * (u2 + 1) + 16.0 * a2 + 4.0 * u2))
            generic_bytes = lift_bytes + agg_bytes
            line["graph_build_roofline"] = {
                "what": "fused order-2 De Bruijn builder (event records, 2 radix sorts of the events, per-node passes, CSR of both layers incl. gcn_norm "
                        "and the bipartite grouping): bytes it really moves = events in + plans out, over its kernels' time (pp_debruijn2_lists .. _fill)",
                "kernel": fkey, "avg_ms": f_avg, "bytes_moved": moved,
                "achieved": moved / (f_avg * 1e-3) / 1e9 if f_avg > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": (moved / (f_avg * 1e-3) / 1e9 / HBM_PEAK_GBS) if f_avg > 0 else 0.0,
                "bound": "latency / instruction issue of the per-node waves and ~1.2e8 random accesses, not bytes (DESIGN §5)",
                "generic_pipeline_equivalent": {
                    "what": "SURVEY §8d bytes of what the builder REPLACES (lift 24 m + 16 E2, both aggregations) over the builder's time: an "
                            "equivalent-work speed for comparison with lift_roofline / aggregation_roofline, not bandwidth the builder reaches",
                    "algorithmic_bytes": generic_bytes, "GB_per_s": generic_bytes / (f_avg * 1e-3) / 1e9 if f_avg > 0 else 0.0}}
        if args.full and not args.no_cpu_baseline and world == 1:
            line["cpu_baseline"] = cpu_baseline_isolated(args)
        print(json.dumps(line), flush=True)
    if launched:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
