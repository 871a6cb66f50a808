"""Random walks on a :class:`~pathpyg_amd.Graph` or on a layer of a :class:`~pathpyg_amd.MultiOrderModel`, sampled on the GPU
(``csrc/pp_walks.hip``; the header's "random walks" block is the contract, ``tests/cpu_ops_walks.py`` restates it).

The generative half of the package: walks from layer ``k`` of a model are the null model ``estimate_order`` should hand back as order
``k``, and a :class:`WalkBatch` packs into the :class:`~pathpyg_amd.PathData` the builders read, without leaving the device.  ``W`` walks are
``W`` independent pointer chases, one lane each; every walk is a pure function of ``(seed, graph, weights, arguments)`` — the same bits on
every run, whatever the grid.

A walk moves from ``v`` along one of its stored out-edges, chosen with probability ``weight / (sum of v's weights)`` (parallel edges are
separate entries; an edge of weight 0 is never taken), and ends early at a node without an out-edge of positive weight.

Out of scope: restart or teleport, stationary distributions, alias tables, temporal walks on event streams.

Randomness follows :mod:`~pathpyg_amd.algorithms.generative_models`: ``seed=None`` draws one int64 from torch's default CPU generator, so
``torch.manual_seed`` makes a script reproducible; the seed used is kept in ``pathpyg_amd.processes.last_seed``.  Negative seeds are taken
modulo 2^64.  There is no CPU fallback: a host-resident graph is moved to the compute device.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _dispatch, _hip
from ..core.graph import Graph
from ..core.index_map import IndexMap
from ..core.path_data import PathData

last_seed = None             # the seed of the most recent RandomWalk.run


class UnknownEdgeAttribute(AttributeError, ValueError):
    """An edge attribute the graph does not have: the ``AttributeError`` of ``Graph.degrees``, and an argument error like the others here."""


def _seed(seed) -> int:
    global last_seed
    if seed is None:
        seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64).item())
    last_seed = int(seed)
    return last_seed & 0xFFFFFFFFFFFFFFFF


class WalkBatch:
    """The walks of one :meth:`RandomWalk.run`, on the device.

    ``nodes``: int64 ``[W, steps + 1]``, the visited nodes of the graph walked on (layer-node indices for a higher-order layer), ``-1``
    after a walk's end; made on first access from the step-major int32 buffer the kernel wrote (``steps_major``, ``[steps + 1, W]``).
    ``lengths``: int64 ``[W]``, edges per walk."""

    def __init__(self, steps_major: torch.Tensor, lengths: torch.Tensor, node_sequence: torch.Tensor, num_nodes: int, mapping: IndexMap,
                 num_first_order) -> None:
        self.steps_major = steps_major
        self.lengths = lengths.to(torch.int64)
        self._lengths32 = lengths
        self._node_sequence = node_sequence
        self._n = num_nodes
        self._mapping = mapping
        self._num_first_order = num_first_order
        self._nodes = None
        self._store = None

    @property
    def nodes(self) -> torch.Tensor:
        if self._nodes is None:
            self._nodes = self.steps_major.t().to(torch.int64).contiguous()
        return self._nodes

    @property
    def num_walks(self) -> int:
        return int(self.steps_major.size(1))

    def _packed(self) -> "_hip.WalkStore":
        if self._store is None:
            self._store = _hip.walk_pack(self.steps_major, self._lengths32, self._node_sequence, self._n)
        return self._store

    def to_path_data(self) -> PathData:
        """The walks as first-order sequences in a device-resident :class:`~pathpyg_amd.PathData` (every walk with weight 1): for a layer of
        order ``k`` the ``k`` nodes of a walk's first layer node, then the last node of every later one.  Walks without an edge are dropped."""
        s = self._packed()
        out = PathData(self._mapping, device=s.node_sequence.device)
        d = out.data
        d.edge_index, d.node_sequence = s.edge_index, s.node_sequence
        d.dag_weight, d.dag_num_edges, d.dag_num_nodes = s.dag_weight, s.dag_num_edges, s.dag_num_nodes
        d.num_nodes = int(s.node_sequence.size(0))
        return out

    def visit_counts(self) -> torch.Tensor:
        """int64 ``[n first-order nodes]``: how often each first-order node occurs in the packed sequences of :meth:`to_path_data`."""
        seq = self._packed().node_sequence.reshape(-1)
        return _hip.degree(seq, int(self._num_first_order())).to(torch.int64)


class RandomWalk:
    """Sampler of random walks on ``graph``.

    Args:
        graph: a :class:`~pathpyg_amd.Graph` of any order (a layer of a :class:`~pathpyg_amd.MultiOrderModel` is one)
        weight: the edge attribute that weights the transitions (``"edge_weight"``), ``None``: every stored edge counts 1.  Weights must be
            finite and not negative (``ValueError`` from the first :meth:`run`, or from :meth:`table`)
        first_order_mapping: the :class:`~pathpyg_amd.IndexMap` of the first-order nodes ``graph.data.node_sequence`` names; it becomes the
            mapping of :meth:`WalkBatch.to_path_data`.  Default: the graph's own mapping for a first-order graph, else none (ids are the
            integers of ``node_sequence``)

    The transition table (float64 running sums of every row's weights) is built once, by the first call that needs it, and kept; so are
    the two start tables.  Restart or teleport, stationary distributions, alias tables and temporal walks on event streams are out of scope.
    """

    def __init__(self, graph: Graph, weight: str | None = None, first_order_mapping: IndexMap | None = None) -> None:
        if weight is not None and getattr(graph.data, weight, None) is None:
            raise UnknownEdgeAttribute(f"graph has no edge attribute {weight}")
        self.graph = graph
        self.weight = weight
        self.order = graph.order
        if first_order_mapping is None:
            first_order_mapping = graph.mapping if self.order == 1 else IndexMap()
        self.mapping = first_order_mapping
        self._csr = None
        self._table = None
        self._start_table = None
        self._positive = None
        self._first_order_nodes = None

    # ------------------------------------------------------------------ tables (device)
    def _device_csr(self):
        if self._csr is None:
            g = self.graph
            dev = _dispatch.compute_device(g.data.edge_index)
            seq = _dispatch.plain(g.data.node_sequence).to(dev).to(torch.int64).contiguous()
            if seq.dim() != 2 or seq.size(0) != g.n or seq.size(1) < 1:
                raise ValueError(f"node_sequence must have one row per node, got {tuple(seq.shape)} for {g.n} nodes")
            self._csr = (g.row_ptr.to(dev).contiguous(), g.col.to(dev).contiguous(), seq)
        return self._csr

    def table(self) -> "_hip.WalkTable":
        """The transition table, built on first use (one kernel, one lane per row; one read-back for the weight check)."""
        if self._table is None:
            row_ptr, col, _ = self._device_csr()
            w = None
            if self.weight is not None:
                w = _dispatch.plain(getattr(self.graph.data, self.weight)).to(row_ptr.device).reshape(-1)
                if w.numel() != col.numel():
                    raise ValueError(f"edge attribute {self.weight} has {w.numel()} entries for {col.numel()} edges")
                if w.dtype not in (torch.float32, torch.float64):
                    w = w.to(torch.float64)
                w = w.contiguous()
            table = _hip.walk_table(row_ptr, self.graph.n, col.numel(), w)
            if table.bad:
                raise ValueError(f"edge attribute {self.weight}: transition weights must be finite and not negative")
            self._table = table
        return self._table

    def _num_first_order(self) -> int:
        if self._first_order_nodes is None:
            if self.mapping.has_ids:
                self._first_order_nodes = self.mapping.num_ids()
            else:
                seq = self._device_csr()[2]
                self._first_order_nodes = _hip.minmax(seq)[1] + 1 if seq.numel() else 0
        return self._first_order_nodes

    # ------------------------------------------------------------------ arguments (host)
    def _explicit_starts(self, start) -> torch.Tensor:
        """int64 start indices from a tensor / array of node indices or a list of node IDs; ``ValueError`` outside ``[0, n)``."""
        n = self.graph.n
        if isinstance(start, (torch.Tensor, np.ndarray)):
            idx = torch.as_tensor(start)
            if idx.dtype.is_floating_point or idx.dtype == torch.bool or idx.dim() != 1:
                raise ValueError("start: a one-dimensional tensor of node indices")
            idx = idx.to(torch.int64)
        elif isinstance(start, (list, tuple)):
            if self.graph.mapping.has_ids:
                try:
                    idx = self.graph.mapping.to_idxs(list(start)).to(torch.int64).reshape(-1)
                except KeyError as e:
                    raise ValueError(f"start: unknown node id {e}") from None
            else:
                idx = torch.tensor(list(start), dtype=torch.int64).reshape(-1)
        else:
            raise ValueError('start: "weighted", "uniform", a tensor of node indices or a list of node ids')
        if idx.numel():
            lo, hi = (_hip.minmax(idx) if idx.is_cuda else (int(idx.min()), int(idx.max())))
            if lo < 0 or hi >= n:
                raise ValueError(f"start: node index outside [0, {n})")
        return idx

    def run(self, num_walks: int | None = None, steps: int = 1, start="weighted", seed: int | None = None) -> WalkBatch:
        """Sample walks of at most ``steps`` edges.

        Args:
            num_walks: how many, when the starts are drawn; must be ``None`` with explicit starts (one walk per start)
            steps: the most edges a walk takes; a walk ends early at a node without an out-edge of positive weight
            start: ``"weighted"``: a start node is drawn with probability proportional to its weight sum (its out-degree without
                weights) — for a layer of a multi-order model, proportional to how often the walks it was built from left that node;
                ``"uniform"``: uniformly among the nodes with a positive weight sum; a tensor / array of node INDICES; a list of node IDS
                (looked up in the graph's mapping; indices if it has none)
            seed: the 64-bit seed; ``None`` draws one from torch's default CPU generator (kept in ``processes.last_seed``)
        """
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
            raise ValueError("steps must be an integer >= 0")
        steps = int(steps)
        drawn = isinstance(start, str)
        if drawn:
            if start not in ("weighted", "uniform"):
                raise ValueError('start: "weighted", "uniform", a tensor of node indices or a list of node ids')
            if num_walks is None:
                raise ValueError("num_walks is needed when the start nodes are drawn")
            if isinstance(num_walks, bool) or not isinstance(num_walks, (int, np.integer)) or num_walks < 0:
                raise ValueError("num_walks must be an integer >= 0")
            walks, given = int(num_walks), None
        else:
            if num_walks is not None:
                raise ValueError("give either num_walks or explicit start nodes, not both")
            given = self._explicit_starts(start)
            walks = int(given.numel())
        g = self.graph
        n, m = g.n, int(g.data.peek("edge_index").shape[1])
        _hip.walk_check_sizes(n, m, walks, steps, self.order)            # refusals by arithmetic, before anything is allocated
        seed = _seed(seed)

        row_ptr, col, node_sequence = self._device_csr()
        table = self.table()
        dev = row_ptr.device
        start_table = positive = None
        if given is not None:
            mode, given = _hip.WALK_START_GIVEN, given.to(dev).contiguous()
        elif start == "weighted":
            mode = _hip.WALK_START_WEIGHTED
            if self._start_table is None:
                bcum, B = _hip.walk_start_table(table.total)
                self._start_table = (bcum, B, float(B[-1].item()) if B.numel() else 0.0)
            if not self._start_table[2] > 0.0:
                raise ValueError("no node has an out-edge of positive weight: there is nowhere to start a walk")
            start_table = self._start_table[:2]
        else:
            mode = _hip.WALK_START_UNIFORM
            if self._positive is None:
                self._positive = _hip.walk_positive_nodes(table.total)
            if self._positive.numel() == 0:
                raise ValueError("no node has an out-edge of positive weight: there is nowhere to start a walk")
            positive = self._positive
        nodes, lengths = _hip.walk_run(row_ptr, col, table, n, walks, steps, self.order, seed, mode, given, start_table, positive)
        return WalkBatch(nodes, lengths, node_sequence, n, self.mapping, self._num_first_order)
