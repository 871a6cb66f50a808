"""Random walks on a :class:`~pathpyg_amd.Graph` or on a layer of a :class:`~pathpyg_amd.MultiOrderModel`, sampled on the GPU
(``csrc/pp_walks.hip``; the header's "random walks" block is the contract, ``tests/cpu_ops_walks.py`` restates it).

The generative half of the package: walks from layer ``k`` of a model are the null model ``estimate_order`` should hand back as order
``k``, and a :class:`WalkBatch` packs into the :class:`~pathpyg_amd.PathData` the builders read, without leaving the device.  ``W`` walks are
``W`` independent pointer chases, one lane each; every walk is a pure function of ``(seed, graph, weights, arguments)`` — the same bits on
every run, whatever the grid.

A walk moves from ``v`` along one of its stored out-edges, chosen with probability ``weight / (sum of v's weights)`` (parallel edges are
separate entries; an edge of weight 0 is never taken), and ends early at a node without an out-edge of positive weight.

The deterministic half runs on the batched propagator of ``csrc/pp_graph_diffusion.hip`` (the header's "distributions and PageRank" block):
:meth:`RandomWalk.evolve` pushes B start distributions through the same chain — where the probability mass is after ``t`` steps, the total
variation distance to a target over time — and :meth:`RandomWalk.stationary_distribution` iterates to the fixed point; both project onto
first-order nodes (:meth:`RandomWalk.first_order`).  Mass that reaches a node without an out-edge of positive weight stays there, which is
what :meth:`RandomWalk.run` does with a walk.  Teleport lives in :func:`pathpyg_amd.algorithms.pagerank`.

Out of scope: alias tables, temporal walks on event streams.

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
    the two start tables, the propagator's pull structure and the first-order grouping.  Alias tables and temporal walks on event streams
    are out of scope.
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
        self._structure = None
        self._grouping = None

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

    # ------------------------------------------------------------------ distributions (csrc/pp_graph_diffusion.hip)
    def structure(self):
        """``(col_ptr, src, _hip.DiffusionTable)``: the pull structure of the propagator over the graph's MERGED entries, built on first use
        and kept.  An entry weighs its parallel edges' weights summed — the number of stored edges behind it with ``weight=None`` — so the
        chain is the one :meth:`run` samples."""
        if self._structure is None:
            structure = _dispatch.graph_diffusion_structure(self.graph, self.weight, count_stored=True)
            if structure[2].bad:
                raise ValueError(f"edge attribute {self.weight}: transition weights must be finite and not negative")
            self._structure = structure
        return self._structure

    def _first_order_grouping(self):
        """``(ptr [n1 + 1], order [n])``: the layer nodes grouped by their last first-order node, ascending inside a group (the stable
        argsort), made once and kept."""
        if self._grouping is None:
            last = self._device_csr()[2][:, -1].contiguous()
            n1 = self._num_first_order()
            if last.numel() and (_hip.minmax(last)[0] < 0 or _hip.minmax(last)[1] >= n1):
                raise ValueError(f"node_sequence names first-order nodes outside [0, {n1})")
            order = _hip.argsort(last, (0, max(n1 - 1, 0))) if last.numel() else last
            self._grouping = (_hip.ptr_from_sorted(last[order], n1), order)
        return self._grouping

    def first_order(self, values, *, heavy_min: int = 0) -> torch.Tensor:
        """The projection of a block on the graph's nodes (``[n]`` or ``[n, B]``) onto first-order nodes: float64 ``[n1]`` / ``[n1, B]`` on the
        device, ``first[v1] = sum of values[u]`` over the nodes ``u`` whose last first-order node (``node_sequence[u, -1]``) is ``v1``,
        in ascending ``u``.  The identity for a first-order graph."""
        values = torch.as_tensor(values)
        if values.dim() not in (1, 2) or values.size(0) != self.graph.n:
            raise ValueError(f"values must be [n] or [n, B] with n = {self.graph.n}, got {tuple(values.shape)}")
        ptr, order = self._first_order_grouping()
        block = values.reshape(self.graph.n, -1).to(ptr.device).to(torch.float64)
        if block.size(1) == 0:
            return torch.empty((self._num_first_order(), 0), dtype=torch.float64, device=ptr.device)
        out = _dispatch.diffusion_project(ptr, order, self._num_first_order(), block, heavy_min)
        return out.reshape(-1) if values.dim() == 1 else out

    def _total_weight(self) -> float:
        """The sum of all T_v, in the fixed shape of the projection kernel (one group that holds every node)."""
        total = self.structure()[2].total
        n = total.numel()
        ptr = torch.tensor([0, n], dtype=torch.int64, device=total.device)
        return float(_dispatch.diffusion_project(ptr, torch.arange(n, dtype=torch.int64, device=total.device), 1, total.reshape(-1, 1)).item())

    @staticmethod
    def _start_width(start) -> int:
        """The number of columns a start argument asks for, from its form alone (host code)."""
        if isinstance(start, str):
            if start not in ("weighted", "uniform"):
                raise ValueError('start: "weighted", "uniform", node indices or ids, or a float [n] / [n, B] distribution')
            return 1
        if isinstance(start, (torch.Tensor, np.ndarray)):
            t = torch.as_tensor(start)
            if t.dtype.is_floating_point:
                if t.dim() not in (1, 2):
                    raise ValueError(f"a start distribution is [n] or [n, B], got {tuple(t.shape)}")
                return 1 if t.dim() == 1 else int(t.size(1))
            if t.dim() != 1 or t.dtype == torch.bool:
                raise ValueError("start: a one-dimensional tensor of node indices")
            return int(t.numel())
        if isinstance(start, (list, tuple)):
            return len(start)
        raise ValueError('start: "weighted", "uniform", node indices or ids, or a float [n] / [n, B] distribution')

    def _host_start(self, start, name: str = "start"):
        """A start argument checked on the host, as ``(kind, value, squeeze)``: ``("drawn", "weighted" | "uniform", True)``, ``("indices",
        int64 [B], False)`` or ``("block", normalised float64 [n, B] on the host, it had no column axis)``."""
        from ..algorithms.ranking import _checked_weights, normalized_columns
        n = self.graph.n
        if isinstance(start, str):
            return "drawn", start, True
        if isinstance(start, (torch.Tensor, np.ndarray)) and torch.as_tensor(start).dtype.is_floating_point:
            t = torch.as_tensor(start).to(torch.float64).cpu()
            if t.size(0) != n:
                raise ValueError(f"{name}: a distribution has one entry per node ({n}), got shape {tuple(t.shape)}")
            return "block", normalized_columns(_checked_weights(t.reshape(n, -1), name), name), t.dim() == 1
        return "indices", self._explicit_starts(start), False

    def _start_block(self, spec):
        """``(block float64 [n, B] on the device, squeeze)`` of a checked start (:meth:`_host_start`)."""
        kind, value, squeeze = spec
        n = self.graph.n
        table = self.structure()[2]
        dev = table.total.device
        if kind == "block":
            return value.to(dev), squeeze
        if kind == "indices":
            idx = value.to(dev)
            block = torch.zeros((n, idx.numel()), dtype=torch.float64, device=dev)
            block[idx, torch.arange(idx.numel(), device=dev)] = 1.0
            return block, squeeze
        if value == "weighted":
            total = self._total_weight()
            if not total > 0.0:
                raise ValueError("no node has an out-edge of positive weight: there is nowhere to start")
            return (table.total / total).reshape(n, 1), squeeze
        positive = table.total > 0
        count = int(positive.sum().item())
        if count == 0:
            raise ValueError("no node has an out-edge of positive weight: there is nowhere to start")
        return (positive.to(torch.float64) * (1.0 / count)).reshape(n, 1), squeeze

    def _check_process(self, start, lazy, kept: int, name: str = "start"):
        """The refusals that need no device — the forms and values of the arguments, the sizes by arithmetic (nothing is allocated) — and
        ``(lazy, the checked start)``."""
        if isinstance(lazy, bool) or not isinstance(lazy, (int, float, np.integer, np.floating)) or not 0.0 <= float(lazy) <= 1.0:
            raise ValueError(f"lazy must lie in [0, 1], got {lazy!r}")
        g = self.graph
        if g.n == 0:
            raise ValueError("the graph has no nodes: there is no distribution on it")
        width = self._start_width(start)
        if width == 0:
            raise ValueError(f"{name} names no distribution")
        _hip.diffusion_check_sizes(g.n, int(g.data.peek("edge_index").shape[1]), _hip.diffusion_width(min(width, _hip.DIFFUSION_MAX_WIDTH)), kept)
        return float(lazy), self._host_start(start, name)

    def evolve(self, start, steps: int, *, lazy: float = 0.0, target=None, keep_all: bool = False, batch: int = 0,
               heavy_min: int = 0) -> "Evolution":
        """Where the probability mass is after ``steps`` steps of the walk: every start distribution ``x`` is pushed through
        ``x'[v] = lazy * x[v] + (1 - lazy) * (sum_u P[u, v] x[u] + (x[v] if v is dangling))``, ``P[u, v] = w(u, v) / T_u``; a node without
        an out-edge of positive weight is dangling and keeps its mass, as :meth:`run` leaves a walk there.  All ``steps`` iterations are
        enqueued with one synchronisation at the end.

        Args:
            start: ``"weighted"``: ``T_v / sum T``; ``"uniform"``: ``1 / #nodes with T_v > 0`` on those nodes; a tensor / array of node
                INDICES or a list of node IDS: one one-hot column each; a float ``[n]`` or ``[n, B]`` tensor / array: distributions, not
                negative and finite, normalised per column (``ValueError`` for an all-zero column)
            steps: the number of iterations, >= 0
            lazy: the probability of staying put in a step, in [0, 1]
            target: a float ``[n]`` distribution (normalised) or ``"stationary"`` (:meth:`stationary_distribution`, computed with this
                ``lazy``, or with 0.5 if it is 0: the fixed point is the same and periodic chains converge): switches ``tvd`` on
            keep_all: keep every iterate
            batch, heavy_min: kernel settings (0 = the library's choice); they change no bit, respectively only the shape of long rows' sums
        """
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
            raise ValueError("steps must be an integer >= 0")
        steps = int(steps)
        lazy, spec = self._check_process(start, lazy, steps + 1 if keep_all else 2)
        if isinstance(target, str):
            if target != "stationary":
                raise ValueError('target: a float [n] distribution or "stationary"')
        elif target is not None:
            t = torch.as_tensor(target) if isinstance(target, (torch.Tensor, np.ndarray)) else None
            if t is None or t.dim() != 1 or not t.dtype.is_floating_point:
                raise ValueError("target: a float [n] distribution or \"stationary\"")
            target = self._host_start(t, "target")[1].reshape(-1)
        n = self.graph.n
        block, squeeze = self._start_block(spec)
        if isinstance(target, str):
            target = self.stationary_distribution(lazy=lazy if lazy > 0.0 else 0.5)
        run = _dispatch.graph_diffusion(self.structure(), n, _dispatch.DIFFUSION_WALK, block, -1.0, steps, lazy=lazy, target=target,
                                        keep_all=keep_all, want_tvd=target is not None, batch=batch, heavy_min=heavy_min)
        return Evolution(self, run, squeeze, steps)

    def stationary_distribution(self, *, lazy: float = 0.0, tol: float = 1e-12, max_iter: int = 10000, nstart=None, return_iterations: bool = False,
                                batch: int = 0, heavy_min: int = 0):
        """The stationary visitation probabilities: the iteration of :meth:`evolve` from ``nstart`` (its ``start`` forms; default
        ``"weighted"``) until ``sum |x' - x| < tol``.  Float64 ``[n]`` on the device (``[n, B]`` for a start with a column axis); with
        ``return_iterations`` the iteration count follows (a list for ``[n, B]``).  Raises
        :class:`~pathpyg_amd.algorithms.centrality.PowerIterationFailedConvergence` after ``max_iter`` iterations.

        The result is the LIMIT FROM THAT START.  It is the unique stationary distribution if the chain is strongly connected and
        aperiodic; otherwise it depends on the start (mass in different closed classes, or on dangling nodes, stays apart), and a periodic
        chain may not converge at all — ``lazy > 0`` removes periodicity without moving the fixed point (``x P = x`` iff
        ``lazy x + (1 - lazy) x P = x``), at the price of more iterations."""
        from ..algorithms.centrality import PowerIterationFailedConvergence
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
            raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
        if not float(tol) > 0.0:
            raise ValueError(f"tol must be positive, got {tol!r}")
        start = "weighted" if nstart is None else nstart
        lazy, spec = self._check_process(start, lazy, 2, "nstart")
        block, squeeze = self._start_block(spec)
        run = _dispatch.graph_diffusion(self.structure(), self.graph.n, _dispatch.DIFFUSION_WALK, block, float(tol), int(max_iter), lazy=lazy,
                                        batch=batch, heavy_min=heavy_min)
        failed = [c for c, ok in enumerate(run.converged) if not ok]
        if failed:
            raise PowerIterationFailedConvergence(max_iter, None if squeeze else failed)
        values = run.final.reshape(-1) if squeeze else run.final
        if return_iterations:
            return values, (run.iterations[0] if squeeze else run.iterations)
        return values


class Evolution:
    """What :meth:`RandomWalk.evolve` returns, on the device.

    ``final``: float64 ``[n, B]``, ``[n]`` for a string or one-dimensional start.  ``trajectory``: ``[steps + 1, n, B]`` (``[steps + 1, n]``)
    with ``keep_all``, else ``None``.  ``tvd``: ``[steps + 1, B]`` (``[steps + 1]``), ``tvd[t] = 0.5 * sum |x_t - target|``, with a target,
    else ``None``.  ``iterations`` = ``steps``."""

    def __init__(self, walk: RandomWalk, run, squeeze: bool, steps: int) -> None:
        self._walk = walk
        self.iterations = steps
        self.final = run.final.reshape(-1) if squeeze else run.final
        self.trajectory = run.trajectory
        self.tvd = run.tvd
        if squeeze:
            self.trajectory = None if run.trajectory is None else run.trajectory[:, :, 0]
            self.tvd = None if run.tvd is None else run.tvd[:, 0]

    def first_order(self, trajectory: bool = False) -> torch.Tensor:
        """``final`` — with ``trajectory=True`` every kept iterate — projected onto first-order nodes (:meth:`RandomWalk.first_order`):
        ``[n1, B]`` / ``[steps + 1, n1, B]``, without the column axis where ``final`` has none."""
        if not trajectory:
            return self._walk.first_order(self.final)
        if self.trajectory is None:
            raise ValueError("the trajectory was not kept: evolve(..., keep_all=True)")
        return torch.stack([self._walk.first_order(x) for x in self.trajectory])
