"""Random graph models sampled on the device (reference src/pathpyG/algorithms/generative_models.py).

The reference walks all n^2 pairs in Python for G(n,p) and the stochastic block model and keeps a ``set`` with two ``IndexMap`` lookups per
draw for G(n,m).  Here the edge list is made by the kernels of csrc/pp_random_graphs.hip in work proportional to the edges produced, and
it never passes through the host.  Names and signatures are the reference's; every sampling function takes two more keyword-only
arguments, ``seed`` and ``device``.

**The random stream is a defined pure function.**  The edge set depends on ``(seed, arguments)`` alone — not on the grid, on
``launch_share``, on the device or on the batches the host loop happens to use.  The generator is Philox4x32-10 keyed by the 64-bit seed
(negative seeds count modulo 2^64); the counter layout, the fixed-point widths and the integer-only path from a random word to an edge
are written down in DESIGN.md ("Random graph models"), and tests/cpu_ops_generative.py restates all of it with Python ints, bit for bit.
The two constants a model hands to the device, :func:`skip_constant` and :func:`chunk_log2`, are host float arithmetic on ``p``
(``log1p``): the same platform gives the same graph.  ``seed=None`` draws one int64 from torch's default CPU generator, so
``torch.manual_seed`` makes a script reproducible; the seed used is kept in :data:`last_seed`.

**Results.**  For the sampled edge set the graph equals ``Graph.from_edge_list(edges, is_undirected=not directed, mapping=mapping)`` of
this package in ``n``, ``m``, mapping, ``is_undirected()`` and the set of stored edges — the reference's explicit ``p == 0.0`` case (an
empty graph without nodes and with an empty mapping) and every other empty edge set included.  The default mapping is
``IndexMap([str(i) for i in range(n)])``.  Stored order is row-sorted with ascending columns (``_row_sorted=True``, nothing is re-checked);
undirected results store both directions and carry the flags ``to_undirected()`` sets.  **The result lives on ``device``; with ``None`` it
stays on the compute device (the GPU) where it was made — the reference returns host graphs.**  An EMPTY edge set, from any of the models
(``p == 0``, ``m == 0``, ``n * s == 0``, or a sample that drew nothing), is exactly ``Graph.from_edge_list([], device=device)``: no nodes, an
empty mapping, ``is_undirected()`` False, and — nothing having been made on a device — on the host when ``device`` is ``None``.

**Deviations from the reference**, all deliberate:

* *Stochastic block model:* ``M`` must be symmetric (``ValueError`` otherwise).  The reference reads ``M[z[u], z[v]]`` for ``v < u``, so an
  asymmetric ``M`` makes an undirected edge's probability depend on the index order of its ends.  Entries outside [0, 1] and entries of
  ``z`` outside the matrix are refused as well.
* *G(n,m), ``self_loops=True``, undirected:* the reference picks a loop half as often as any other pair; here every slot is equally likely,
  so the model is uniform over the graphs with m edges.
* *G(n,m), ``multi_edges=True``:* the reference collapses duplicates in its ``set`` and returns fewer than m edges; here m i.i.d. slots are
  returned and duplicates are stored as parallel edges.
* *Watts-Strogatz repairs* (``allow_duplicate_edges=False`` / ``allow_self_loops=False``): the reference's sequential Python loops become
  repair rounds — find the surplus copies of an edge and the loops by sort and adjacent compare, redraw one endpoint from the counter of
  (edge, round), repeat until there are none.  Odd rounds keep the stored first end and redraw the second (what the reference's loop
  does), even rounds keep the second: an edge whose first end has no free partner left would otherwise be redrawn forever.  The outcome is a pure function of the seed but need not be what the reference's
  loop would give for the same draws (that loop has no defined draw order to match).  A redrawn edge is re-oriented (ends sorted) only
  in the undirected case; requests that cannot be met at all are refused instead of looping forever.  The result always has ``n`` nodes.
* *Smallest p:* the skip constant has 32 fraction bits and must stay below 2^32, so ``0 < p <`` :data:`MIN_P` ``= 2^-30`` is refused
  (``ValueError``) rather than sampled wrongly.

``erdos_renyi_gnp_likelihood`` keeps the reference's exponent ``graph.n`` on ``p`` (the likelihood proper has ``graph.m`` there, as the
log-likelihood does): it is a quirk of the reference and kept so that results agree.  The three likelihood functions are host arithmetic.

**Degree-sequence models** (``is_graphic_erdos_gallai``, ``generate_degree_sequence``, ``molloy_reed``, ``molloy_reed_randomize``,
``k_regular_random``).  The reference matches stubs one pair at a time, tests ``(v, w) in edges`` on a Python list and breaks up a random
edge when a draw fails.  Here all stubs are shuffled at once (a sort by 64-bit keys of the stream) and neighbours are joined; loops and
surplus copies are then repaired in rounds: every offender draws a victim edge, the smallest offender that drew an edge claims it, an
offender acts when it holds its claim and nobody drew it, and exchanges one end with its victim if that leaves no more loops and
duplicates among the two edges than before.  Like everything else here the result is a pure function of ``(seed, arguments)``; DESIGN.md
("Degree-sequence models") has the rules and tests/cpu_ops_degree_models.py restates them.  Deviations, all deliberate:

* *Distribution:* only the first matching is exactly uniform (over stub matchings).  The repaired result is NOT uniform over the simple
  graphs of the sequence — neither is the reference's loop — and is not the reference's distribution.
* *Termination* of the repair rounds is not proven for every graphic sequence; ``MAX_REPAIR_ROUNDS`` rounds end in a ``RuntimeError``.
* *All n nodes are there*, those of degree 0 included; the reference builds the graph from its edge list and loses them.  (An empty edge
  set is the empty graph, as everywhere in this module.)  Without ``node_ids`` the IDs are the ints ``0 .. n - 1`` as in the reference,
  not the ``str`` IDs of the other models.
* *``node_ids`` of the wrong length* is a ``ValueError``; the reference silently ignores the list.
* *``relax=True``* is one matching without repair, loops dropped and duplicates merged — what the reference's docstring describes.  The
  reference's code still breaks up an edge on every loop it draws and appends duplicates to its list.
* *``multiedge=True``* stores parallel edges and repairs only loops.
* *A single node of even positive degree* is not graphic (the condition is applied for r = 1 .. n; the reference stops at n - 1, says True
  and its ``molloy_reed([2])`` never returns).  Degrees that are not finite integers are a ``ValueError``.
* *``generate_degree_sequence``* draws from a seeded ``numpy.random.default_rng`` and gives up after ``MAX_SEQUENCE_TRIES`` draws.
* Degrees summing to 2^31 - 1 or more are refused: stub and edge indices are int32 in the sort.
"""
from __future__ import annotations

import logging
import math
from typing import Optional

import numpy as _np
import torch

from .. import _dispatch
from ..core.graph import Graph
from ..core.index_map import IndexMap
from ..data import Data

logger = logging.getLogger("pathpyg_amd")

CHUNK_EDGES = 128            # expected edges of one chunk of a region (one Philox stream, walked by one lane); tests patch it
GNM_BATCH = None             # draws per round of G(n,m); None: the expected number for m distinct values plus four deviations, then doubling
FRAC_BITS = 40               # fraction bits of -log2(u) on the device
C_FRAC_BITS = 32             # fraction bits of the skip constant
MIN_P = 2.0 ** -30           # the smallest positive probability the region sampler takes
MAX_REPAIR_ROUNDS = 1 << 16
MAX_SEQUENCE_TRIES = 1 << 12 # draws of generate_degree_sequence before it gives up
last_seed = None             # the seed of the most recent sampling call of this module
last_repair_rounds = 0       # repair rounds of the most recent molloy_reed call (rounds that found offenders; 0 with relax)

RECT, STRICT, DIAG, NO_DIAG = 0, 1, 2, 3      # region kinds (RG_* of _hip, kReg* of the kernels)


def max_edges(n: int, directed: bool = False, multi_edges: bool = False, self_loops: bool = False) -> int | float:
    """The number of node pairs an edge can join in a network of n nodes, ``np.inf`` once multi-edges are allowed.  The values and types are
    the reference's (an ``int``; the undirected counts go through a float division, so they round beyond 2^53 as the reference's do)."""
    if multi_edges:
        return _np.inf
    closed_form = {                                                    # (directed, self_loops) -> pairs
        (True, True): n * n,
        (True, False): n * (n - 1),
        (False, True): n * (n + 1) / 2,
        (False, False): n * (n - 1) / 2,
    }
    return int(closed_form[bool(directed), bool(self_loops)])


# ------------------------------------------------------------------ host side of the stream definition
def skip_constant(p: float) -> int:
    """``c = -1 / log2(1 - p)`` with :data:`C_FRAC_BITS` fraction bits, truncated; 0 for ``p >= 1`` (every slot is taken)."""
    if p >= 1.0:
        return 0
    return int(-1.0 / (math.log1p(-p) / math.log(2.0)) * 2.0 ** C_FRAC_BITS)


def chunk_log2(p: float, chunk_edges: int | None = None) -> int:
    """log2 of the slots of a chunk: the smallest power of two with ``chunk_edges`` expected edges or more (at most 2^62)."""
    want = CHUNK_EDGES if chunk_edges is None else chunk_edges
    k = 0
    while k < 62 and math.ldexp(p, k) < want:
        k += 1
    return k


def check_probability(p: float, what: str = "p") -> float:
    p = float(p)
    if not 0.0 <= p <= 1.0:                                            # (a NaN fails both comparisons)
        raise ValueError(f"{what} must lie in [0, 1], got {p}")
    if 0.0 < p < MIN_P:
        raise ValueError(f"{what} = {p} is below the smallest supported probability 2^-30: the skip constant would leave its 32.32 fixed-point format")
    return p


def slot_space(n: int, directed: bool, self_loops: bool) -> tuple[int, int, int]:
    """``(N, kind, cols)`` of the pair slots of n nodes, in exact integers."""
    if directed:
        return (n * n, RECT, n) if self_loops else (n * (n - 1), NO_DIAG, max(n - 1, 0))
    return (n * (n + 1) // 2, DIAG, 0) if self_loops else (n * (n - 1) // 2, STRICT, 0)


def region_table(regions: list) -> tuple[list, int]:
    """``(rows, n_chunks)``: the int64 ``[R, 8]`` descriptor rows of ``[(N, p, kind, cols, row_off, col_off), ...]`` (see the C header)
    and the total number of chunks.  A region without slots or with ``p == 0`` gets no chunk."""
    rows, chunk = [], 0
    for N, p, kind, cols, row_off, col_off in regions:
        if N <= 0 or p <= 0.0:
            rows.append([chunk, 0, 0, 0, kind, cols, row_off, col_off])
            continue
        k = chunk_log2(p)
        rows.append([chunk, N, k, skip_constant(p), kind, cols, row_off, col_off])
        chunk += (N + (1 << k) - 1) >> k
    return rows, chunk


def block_regions(M: _np.ndarray, sizes: list) -> list:
    """The B (B + 1) / 2 regions of a block model in rank space (nodes stably sorted by block): block a against block b <= a."""
    offsets = [0]
    for s in sizes:
        offsets.append(offsets[-1] + s)
    regions = []
    for a in range(len(sizes)):
        for b in range(a + 1):
            p = float(M[a, b])
            if a == b:
                regions.append((sizes[a] * (sizes[a] - 1) // 2, p, STRICT, 0, offsets[a], offsets[a]))
            else:
                regions.append((sizes[a] * sizes[b], p, RECT, sizes[b], offsets[a], offsets[b]))
    return regions


def rewire_threshold(p: float) -> tuple[int, bool]:
    """``(floor(p * 2^64), always)``: an edge is rewired when its 64-bit decision draw is below the threshold (``always`` for p >= 1)."""
    p = float(p)
    if p >= 1.0:
        return 0, True
    return (int(math.ldexp(p, 64)) if p > 0.0 else 0), False


def gnm_first_batch(N: int, k: int) -> int:
    """Draws of the first round for k distinct values below N: the expected number plus four standard deviations (roughly) plus 16."""
    if GNM_BATCH is not None:
        return max(int(GNM_BATCH), 1)
    expect = -N * math.log1p(-k / N) if k < N else N * (math.log(N) + 1.0)
    return int(expect + 4.0 * math.sqrt(expect) + 16.0)


def _seed(seed) -> int:
    global last_seed
    if seed is None:
        seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64).item())
    last_seed = int(seed)
    return last_seed & 0xFFFFFFFFFFFFFFFF


def _mapping(mapping, n: int) -> IndexMap:
    if mapping is None:
        return IndexMap([str(i) for i in range(n)])                    # indices for all n nodes, with or without incident edges
    if mapping.num_ids() < n:
        raise ValueError(f"mapping holds {mapping.num_ids()} node IDs, fewer than n = {n}")
    return mapping


def _empty(device) -> Graph:
    """The result for an empty edge set (module docstring): what ``from_edge_list`` makes of no edges."""
    return Graph.from_edge_list([], device=device)


def _finish(edge_index: torch.Tensor, n: int, mapping, directed: bool, device, row_sorted: bool, multi: bool = False) -> Graph:
    """The Graph of a sampled edge list on the compute device: (row, col)-sorted, mirrored when undirected (one stored loop per loop)."""
    if edge_index.size(1) == 0:
        return _empty(device)
    num_nodes = n if mapping is None else mapping.num_ids()
    if directed:
        ei = edge_index if row_sorted else _dispatch.random_sort_edges(edge_index, n)
    elif multi:
        mirror = edge_index.flip(0)[:, edge_index[0] != edge_index[1]]
        ei = _dispatch.random_sort_edges(torch.cat((edge_index, mirror), dim=1), n)
    else:
        ei, _ = _dispatch.coalesce(torch.cat((edge_index, edge_index.flip(0)), dim=1), None, n)
    g = Graph(Data(edge_index=ei, num_nodes=num_nodes), mapping, _row_sorted=True)
    if not directed:
        g.is_undirected_flag = True
        g.data.edge_index.is_undirected = True
    return g if device is None else g.to(device)


# ------------------------------------------------------------------ G(n,p)
def erdos_renyi_gnp(n: int, p: float, mapping: IndexMap | None = None, self_loops: bool = False, directed: bool = False, *,
                    seed: int | None = None, device=None) -> Graph:
    """An Erdös-Renyi random graph with n nodes and link probability p (the G(n,p) model of Gilbert).

    Args:
        n: the number of nodes
        p: the link probability: 0, or between 2^-30 and 1
        mapping: optional mapping of n nodes to node IDs; default ``IndexMap([str(i) for i in range(n)])``
        self_loops: whether self-loops (v, v) may be generated
        directed: whether to generate a directed graph
        seed: the 64-bit seed of the stream; ``None`` draws one from torch's default CPU generator (kept in :data:`last_seed`)
        device: where the result lives; ``None``: on the compute device where it was made (the reference returns host graphs)
    """
    seed = _seed(seed)
    p = check_probability(p)
    mapping = _mapping(mapping, n)
    if p == 0.0:                                                       # the reference's special case: no edges, no nodes
        return _empty(device)
    N, kind, cols = slot_space(n, directed, self_loops)
    rows, n_chunks = region_table([(N, p, kind, cols, 0, 0)])
    edge_index = _dispatch.random_regions(rows, n_chunks, seed, n, device=device)
    return _finish(edge_index, n, mapping, directed, device, row_sorted=True)


def erdos_renyi_gnp_randomize(graph: Graph, self_loops: bool = False, *, seed: int | None = None, device=None) -> Graph:
    """A G(n,p) graph whose nodes, expected number of edges, directedness and node IDs match the given graph's."""
    directed = graph.is_directed()
    density = graph.m / max_edges(graph.n, directed, False, self_loops)            # edges per pair slot: the p that reproduces m in expectation
    return erdos_renyi_gnp(graph.n, density, graph.mapping, self_loops, directed, seed=seed, device=device)


# ------------------------------------------------------------------ G(n,m)
def _first_distinct(N: int, k: int, seed: int, device) -> torch.Tensor:
    """The first k distinct values of the draw sequence d_0, d_1, ... below N, ascending: draw a batch, sort (value, draw index), keep first
    occurrences, take the k of smallest draw index; extend the batch while fewer than k are distinct (one read-back per round)."""
    batch = gnm_first_batch(N, k)
    values = None
    while True:
        drawn = 0 if values is None else values.numel()
        if drawn + batch >= 0x7fffffff:
            raise ValueError("erdos_renyi_gnm: 2^31 - 1 or more draws (draw indices are int32 in the sort)")
        new = _dispatch.random_draws(N, seed, drawn, batch, device=device)
        values = new if values is None else torch.cat((values, new))
        distinct, slots = _dispatch.random_first_distinct(values, k, N.bit_length())
        if slots is not None:
            return slots
        if GNM_BATCH is None:
            batch = values.numel()


def erdos_renyi_gnm(n: int, m: int, mapping: IndexMap | None = None, self_loops: bool = False, multi_edges: bool = False,
                    directed: bool = False, *, seed: int | None = None, device=None) -> Graph:
    """A random graph with n nodes and m edges, uniform over such graphs (the G(n,m) model of Erdös and Renyi).

    The edge slots are the first m distinct values of an infinite sequence of unbiased draws below N = ``max_edges(...)`` (multiply-high
    with rejection) — the reference's sequential process, which does not depend on batch sizes.  For ``m > N / 2`` the ``N - m`` excluded
    slots are sampled by the same rule and the complement is emitted.  With ``multi_edges`` the m draws themselves are the edges.
    See the module docstring for the two deviations (loop weighting, multi-edges) and for ``seed`` / ``device``.
    """
    N, kind, cols = slot_space(n, directed, self_loops)
    limit = max_edges(n, directed, multi_edges, self_loops)
    if limit < m or (m > 0 and (N == 0 or (m > N and not multi_edges))):              # (the second test: exact, where the float limit rounds)
        raise ValueError(f"m = {m} edges exceed the theoretical maximum of a graph with n = {n} nodes ({N} pair slots)")
    seed = _seed(seed)
    mapping = _mapping(mapping, n)
    m = int(m)
    if m <= 0:
        return _empty(device)
    if multi_edges:
        slots = _dispatch.random_sorted(_dispatch.random_draws(N, seed, 0, m, device=device), N.bit_length())
    elif 2 * m <= N:
        slots = _first_distinct(N, m, seed, device)
    else:
        slots = _dispatch.random_complement(_first_distinct(N, N - m, seed, device) if m < N else None, N, device=device)
    return _finish(_dispatch.random_decode(slots, kind, cols), n, mapping, directed, device, row_sorted=True, multi=multi_edges)


def erdos_renyi_gnm_randomize(graph: Graph, self_loops: bool = False, multi_edges: bool = False, *, seed: int | None = None,
                              device=None) -> Graph:
    """A G(n,m) graph whose nodes, edges, directedness and node IDs match the given graph's."""
    return erdos_renyi_gnm(graph.n, graph.m, directed=graph.is_directed(), self_loops=self_loops, multi_edges=multi_edges,
                           mapping=graph.mapping, seed=seed, device=device)


# ------------------------------------------------------------------ stochastic block model
def check_block_matrix(M) -> _np.ndarray:
    M = _np.asarray(M, dtype=_np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError(f"the block matrix must be square, got shape {M.shape}")
    if not (M == M.T).all():
        raise ValueError("the block matrix must be symmetric: the graph is undirected (the reference reads M[z[u], z[v]] for v < u only)")
    for a in range(M.shape[0]):
        for b in range(a + 1):
            check_probability(M[a, b], f"M[{a}, {b}]")
    return M


def stochastic_block_model(M, z, mapping: Optional[IndexMap] = None, *, seed: int | None = None, device=None) -> Graph:
    """A random undirected graph of the stochastic block model: nodes u != v are linked with probability ``M[z[u], z[v]]``.

    Args:
        M: symmetric B x B matrix of probabilities (0, or between 2^-30 and 1)
        z: block assignment vector, ``z[i]`` in 0 .. B-1 the block of the i-th node; its length is the number of nodes
        mapping: optional mapping of node IDs; default ``IndexMap([str(i) for i in range(n)])``

    All block pairs are sampled in ONE launch: the nodes are stably sorted by block, block pair (a, b <= a) is a region of that rank space,
    and the chunks of all regions form one table.  Ranks are mapped back to node indices when the edges are written.
    """
    seed = _seed(seed)
    M = check_block_matrix(M)
    z = z if isinstance(z, torch.Tensor) else torch.as_tensor(_np.asarray(z))
    if z.dim() != 1 or (z.numel() > 0 and (z.is_floating_point() or z.is_complex())):
        raise ValueError("z must be a vector of integer block indices")
    n = z.numel()
    mapping = _mapping(mapping, n)
    if n == 0:
        return _empty(device)
    z = z.to(torch.int64)
    # the range check reads z where it lives: a host vector on the host (no device is needed to refuse it), a device vector by one kernel
    lo, hi = _dispatch.minmax(z) if z.is_cuda else (int(z.min()), int(z.max()))
    if lo < 0 or hi >= M.shape[0]:
        raise ValueError(f"z holds block indices outside the {M.shape[0]} x {M.shape[0]} block matrix")
    sizes, perm = _dispatch.random_block_order(z, M.shape[0], device=device)
    rows, n_chunks = region_table(block_regions(M, sizes))
    edge_index = _dispatch.random_regions(rows, n_chunks, seed, n, device=device, perm=perm)
    return _finish(edge_index, n, mapping, False, device, row_sorted=False)


# ------------------------------------------------------------------ Watts-Strogatz
def watts_strogatz(n: int, s: int, p: float = 0.0, undirected: bool = True, allow_duplicate_edges: bool = True,
                   allow_self_loops: bool = True, mapping: IndexMap | None = None, *, seed: int | None = None, device=None) -> Graph:
    """A Watts-Strogatz small-world graph: the ring lattice of n nodes with s neighbours each, every edge rewired to a uniform target
    with probability p.

    Args:
        n: the number of nodes
        s: the number of ring neighbours every node links to
        p: the rewiring probability
        undirected: orient every edge (ends sorted) and return the undirected graph
        allow_duplicate_edges: ``False`` redraws surplus copies of an edge until there are none
        allow_self_loops: ``False`` redraws loops until there are none
        mapping: node IDs; ``None`` leaves the graph without IDs, as the reference does
    """
    n, s = int(n), int(s)
    count = n * s
    slots = slot_space(n, not undirected, allow_self_loops)[0]
    if not allow_duplicate_edges and count > min(slots, n * (n - 1)):              # (n (n - 1): the bound the reference tests)
        raise ValueError(f"n * s = {count} distinct edges do not fit into a graph of {n} nodes; pass `allow_duplicate_edges=True` to allow copies")
    if not allow_self_loops and count > 0 and n < 2:
        raise ValueError("a graph of one node has no edge that is not a self-loop")
    seed = _seed(seed)
    if count <= 0:
        return _empty(device)
    threshold, always = rewire_threshold(p)
    edge_index = _dispatch.random_ring(n, s, seed, threshold, always, undirected, not allow_duplicate_edges, not allow_self_loops,
                                       MAX_REPAIR_ROUNDS, device=device)
    g = _finish(edge_index, n, None, not undirected, None, row_sorted=False)      # (undirected: parallel edges merge, as in to_undirected())
    if mapping is not None:
        g.mapping = mapping
    return g if device is None else g.to(device)


# ------------------------------------------------------------------ degree-sequence models
def _degree_vector(degrees) -> torch.Tensor:
    """The int64 vector of a list, numpy array or tensor of degrees, where the input lives.  Floating-point entries must be finite and
    integral (``ValueError``); magnitudes beyond 2^62 are clamped, which changes no answer (no sequence holding one is graphic)."""
    t = degrees if isinstance(degrees, torch.Tensor) else torch.as_tensor(_np.asarray(degrees))
    if t.dim() != 1 or t.is_complex() or t.dtype == torch.bool:
        raise ValueError("a degree sequence is a vector of integers")
    if t.is_floating_point():
        if t.numel() > 0 and not bool(torch.isfinite(t).all()):
            raise ValueError("a degree sequence holds finite integers (found inf or nan)")
        if t.numel() > 0 and bool((t != t.round()).any()):
            raise ValueError("a degree sequence holds integers (found a fractional entry)")
        t = t.to(torch.float64).clamp(-2.0 ** 62, 2.0 ** 62)
    return t.to(torch.int64)


def is_graphic_erdos_gallai(degrees) -> bool:
    """Whether a simple undirected graph with these node degrees exists: the condition of Erdös and Gallai (1960) for r = 1 .. n on the
    descending sequence, an even sum and no negative entry.

    ``degrees`` is a list, numpy array or tensor, on the host or the device; floating-point entries must be finite and integral
    (``ValueError`` otherwise).  The degrees are sorted on the device and one lane tests each r (``k_eg_check``) — the reference runs
    two nested Python loops.  ``[]`` is graphic.  Unlike the reference (which stops at r = n - 1) a single node of even positive degree is
    not: the reference's ``molloy_reed([2])`` never returns.
    """
    d = _degree_vector(degrees)
    if d.numel() == 0:
        return True
    return _dispatch.random_graphic(_dispatch.random_degrees(d))


def generate_degree_sequence(n: int, distribution, *, seed: int | None = None, **distribution_args) -> _np.ndarray:
    """A random graphic degree sequence of n entries drawn from a degree distribution (a host function; the test is the device's).

    Args:
        n: the number of nodes
        distribution: a dict ``{degree: probability}``, sampled with ``numpy.random.default_rng(seed).choice``, or an object with ``rvs``
            (a frozen scipy.stats distribution), called with ``random_state=`` that generator; non-integer draws are rounded (``rint``)
        seed: the seed of the numpy generator; ``None``: fresh entropy
        **distribution_args: passed on to ``rvs``

    The sequence is redrawn until it is graphic; after :data:`MAX_SEQUENCE_TRIES` failed draws a ``RuntimeError`` is raised (the
    reference loops forever).  Anything else than a dict or an object with ``rvs`` is a ``NotImplementedError``, as in the reference.
    """
    if isinstance(distribution, dict):
        support = list(distribution)
        probs = [distribution[k] for k in support]

        def draw(rng):
            return rng.choice(_np.asarray(support), size=n, p=probs)
    elif hasattr(distribution, "rvs"):
        def draw(rng):
            s = _np.asarray(distribution.rvs(size=n, random_state=rng, **distribution_args))
            return s if _np.issubdtype(s.dtype, _np.integer) else _np.rint(s)
    else:
        raise NotImplementedError()
    rng = _np.random.default_rng(seed)
    for _ in range(MAX_SEQUENCE_TRIES):
        s = draw(rng)
        if is_graphic_erdos_gallai(s):
            return s
    raise RuntimeError(f"generate_degree_sequence: no graphic sequence in {MAX_SEQUENCE_TRIES} draws")


def molloy_reed(degree_sequence, multiedge: bool = False, relax: bool = False, node_ids: Optional[list] = None, *,
                seed: int | None = None, device=None) -> Graph:
    """A random undirected graph without self-loops whose node i has degree ``degree_sequence[i]`` (the configuration model of Molloy and
    Reed), sampled on the device.

    Args:
        degree_sequence: the n node degrees (list, numpy array or tensor, host or device); ``ValueError`` unless graphic
            (:func:`is_graphic_erdos_gallai`), also with ``multiedge`` or ``relax``, and when they sum to 2^31 - 1 or more
        multiedge: parallel edges are allowed and stored; only loops are repaired
        relax: one stub matching without repairs: loops are dropped and parallel edges merged, so the graph may have fewer than
            ``sum(degree_sequence) / 2`` edges and smaller degrees — what the reference's docstring describes
        node_ids: the n node IDs; default the ints ``0 .. n - 1``.  Another length is a ``ValueError``

    The stubs are shuffled by sorting 64-bit keys of the stream and neighbours are joined — a uniform perfect matching of the stubs.
    Loops and surplus copies of an edge are then repaired in rounds of disjoint degree-preserving end swaps with randomly drawn victim
    edges, accepted where they do not make things worse (module docstring; DESIGN.md "Degree-sequence models"); the number of rounds is
    kept in :data:`last_repair_rounds`.  **Termination is not proven** for every graphic sequence: after :data:`MAX_REPAIR_ROUNDS` rounds
    with offenders left a ``RuntimeError`` is raised.  Sparse and heavy-tailed sequences take a handful of rounds; a sequence with a single
    realisation (a complete graph, a star) takes tens to thousands.
    """
    global last_repair_rounds
    d = _degree_vector(degree_sequence)
    n = d.numel()
    if node_ids is not None and len(node_ids) != n:
        raise ValueError(f"node_ids holds {len(node_ids)} IDs for {n} degrees")
    seed = _seed(seed)
    last_repair_rounds = 0
    if n == 0:
        return _empty(device)
    d = _dispatch.random_degrees(d, device)
    if not _dispatch.random_graphic(d):
        logger.error("given degree sequence is not graphic")
        raise ValueError("given degree sequence is not graphic")
    edge_index, last_repair_rounds = _dispatch.random_matching(d, n, seed, bool(multiedge), bool(relax), MAX_REPAIR_ROUNDS)
    if edge_index is None:
        return _empty(device)
    if relax:
        edge_index = edge_index[:, edge_index[0] != edge_index[1]]
    mapping = IndexMap(_np.arange(n) if node_ids is None else list(node_ids))
    return _finish(edge_index, n, mapping, False, device, row_sorted=False, multi=bool(multiedge) and not relax)


def molloy_reed_randomize(graph: Graph, *, seed: int | None = None, device=None) -> Graph:
    """A randomised realisation of an undirected graph's degree sequence (its in-degrees, which count a stored loop once, as the
    reference's ``degree(edge_index[1])`` does) with the graph's node IDs.  The degrees never leave the device."""
    if graph.is_directed():
        logger.error("molloy_reed_randomize is only implemented for undirected graphs")
        raise NotImplementedError("molloy_reed_randomize is only implemented for undirected graphs")
    return molloy_reed(graph.degrees(mode="in", return_tensor=True), node_ids=graph.nodes, seed=seed, device=device)


def k_regular_random(k: int, n: Optional[int] = None, node_ids: Optional[list] = None, *, seed: int | None = None, device=None) -> Graph:
    """A random graph in which every node has degree k: ``molloy_reed([k] * n, node_ids=node_ids)``; ``n`` defaults to ``len(node_ids)``."""
    if k < 0:
        raise ValueError("Degree parameter k must be non-negative")
    if n is None and node_ids is None:
        raise ValueError("You must either pass a list of node ids or a number of nodes to generate")
    if n is None:
        n = len(node_ids)
    return molloy_reed(torch.full((int(n),), int(k), dtype=torch.int64), multiedge=False, relax=False, node_ids=node_ids, seed=seed, device=device)


# ------------------------------------------------------------------ likelihoods (host arithmetic)
def _pairs_and_edges(graph: Graph, caller: str):
    """``(node pairs as scipy's float binom(n, 2), m)`` of an undirected graph; directed graphs are refused as the reference refuses them."""
    if graph.is_directed():
        raise NotImplementedError(f"{caller} is defined for undirected graphs only")
    from scipy.special import binom
    return binom(graph.n, 2), graph.m


def erdos_renyi_gnp_likelihood(p: float, graph: Graph) -> float:
    """The likelihood the reference assigns to link probability p given an undirected graph: a factor ``1 - p`` per absent pair times
    ``p`` to the power ``graph.n``.  That exponent is the number of NODES — a quirk of the reference (the likelihood proper, and the
    log-likelihood below, have the number of edges there) which is kept so that results agree."""
    pairs, m = _pairs_and_edges(graph, "erdos_renyi_gnp_likelihood")
    absent = pairs - m
    return (1 - p) ** absent * p ** graph.n


def erdos_renyi_gnp_log_likelihood(p: float, graph: Graph) -> float:
    """log10 of the G(n,p) likelihood of p given an undirected graph: every edge weighs ``log10 p``, every absent pair ``log10 (1 - p)``
    (±inf or nan at p = 0 and p = 1, as numpy computes them)."""
    pairs, m = _pairs_and_edges(graph, "erdos_renyi_gnp_log_likelihood")
    absent = pairs - m
    return _np.log10(1 - p) * absent + _np.log10(p) * m


def erdos_renyi_gnp_mle(graph: Graph) -> float:
    """The p that maximises the G(n,p) likelihood of an undirected graph: its density, edges per node pair."""
    pairs, m = _pairs_and_edges(graph, "erdos_renyi_gnp_mle")
    return m / pairs
