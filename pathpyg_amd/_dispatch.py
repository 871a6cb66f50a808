"""Bridge between the reference-shaped Python API (tensors on any device) and the HIP kernels.

Rule: results come back on the device of the inputs, like the reference does
(src/pathpyG/algorithms/temporal.py:30-31, lift_order.py:76).  CPU inputs are staged to the current
MI355X, processed by the HIP kernels and copied back (a PCIe round trip — keep data on the GPU for
throughput).  Without a GPU or without the built library every call raises; nothing is computed on the CPU.
"""
from __future__ import annotations

import torch

from . import _hip


def compute_device(*tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError(
            "pathpyg_amd needs an AMD MI355X (gfx950) visible to PyTorch-ROCm: its lifts, sorts and DBGNN layers "
            "run as HIP kernels only and there is no CPU fallback"
        )
    return torch.device("cuda", torch.cuda.current_device())


def plain(t):
    """View a tensor subclass (e.g. an edge index wrapper) as a plain torch.Tensor."""
    if isinstance(t, torch.Tensor) and type(t) is not torch.Tensor:
        return t.as_subclass(torch.Tensor)
    return t


def _stage(dev, *tensors):
    return tuple(t if (t is None or isinstance(t, str)) else plain(t).to(dev) for t in tensors)      # (str: the _hip.UNIT weight marker)


def _back(like: torch.Tensor, *outs):
    res = tuple(o if (o is None or o.device == like.device) else o.to(like.device) for o in outs)
    return res[0] if len(res) == 1 else res


def temporal_lift(edge_index, time, num_nodes: int, delta, n_own=None, id_offset: int = 0):
    dev = compute_device(edge_index, time)
    ei, t = _stage(dev, edge_index, time)
    return _back(edge_index, _hip.temporal_lift(ei, t, num_nodes, delta, n_own, id_offset))


def temporal_bfs(edge_index, time, num_nodes: int, delta):
    dev = compute_device(edge_index, time)
    ei, t = _stage(dev, edge_index, time)
    event_graph = _hip.temporal_lift(ei, t, num_nodes, delta)
    return _hip.temporal_bfs(ei, num_nodes, event_graph)


def temporal_betweenness(edge_index, time, num_nodes: int, delta):
    dev = compute_device(edge_index, time)
    ei, t = _stage(dev, edge_index, time)
    event_graph = _hip.temporal_lift(ei, t, num_nodes, delta)
    return _hip.temporal_betweenness(ei, num_nodes, event_graph)


def _graph_sources(graph, sources, dev):
    """CSR of a Graph (wherever it lives) and the source indices (default: every node), on the compute device."""
    n = graph.n
    row_ptr, col = _stage(dev, graph.row_ptr, graph.col)
    src = torch.arange(n, dtype=torch.int64, device=dev) if sources is None else torch.as_tensor(sources, dtype=torch.int64).reshape(-1).to(dev)
    return row_ptr, col, n, src


def graph_shortest_paths(graph, sources=None):
    """``(dist, pred)`` int32 ``[len(sources), n]`` on the compute device (the dense route)."""
    dev = compute_device(graph.data.edge_index)
    return _hip.graph_bfs_dense(*_graph_sources(graph, sources, dev))


def graph_path_totals(graph, sources=None):
    """``(reach_in [n], dist_in [n], totals [3])`` as Python lists: one read-back, nothing of size n x n anywhere."""
    dev = compute_device(graph.data.edge_index)
    reach_in, dist_in, totals = _hip.graph_bfs_totals(*_graph_sources(graph, sources, dev))
    n = graph.n
    flat = torch.cat((reach_in, dist_in, totals)).tolist()
    return flat[:n], flat[n:2 * n], flat[2 * n:]


def graph_betweenness(graph, sources=None):
    """``(bw float64 [n], reached bool [n])`` on the CPU.  ``OverflowError`` if a searched source has 2**1024 or more shortest paths to
    some node: float64 path counts end there, and nothing computed from an infinite count is returned."""
    dev = compute_device(graph.data.edge_index)
    bw, reached, overflow = _hip.graph_betweenness(*_graph_sources(graph, sources, dev))
    bw, reached, overflow = bw.cpu(), reached.cpu(), overflow.cpu()
    if bool(overflow.any()):
        v = int(overflow.nonzero()[0])
        raise OverflowError(f"betweenness_centrality: node index {v} has 2**1024 or more shortest paths from a source; path counts are "
                            "float64 and end there (the reference counts in unbounded Python ints)")
    return bw, reached


def graph_components(graph, strong: bool, with_stats: bool = False):
    """``(count int64 [1], labels int32 [n], sizes int64 [n])`` on the compute device (csrc/pp_graph_components.hip); with ``with_stats`` also
    the host list ``[rounds, trim sweeps, colour sweeps, backward sweeps]``.  A CPU-resident graph is staged."""
    dev = compute_device(graph.data.edge_index)
    (ei,) = _stage(dev, graph.data.edge_index)
    csr = _stage(dev, graph.row_ptr, graph.col) if strong else None
    csc = _stage(dev, graph.col_ptr, graph.row) if strong else None
    count, labels, sizes, stats = _hip.graph_components(ei, graph.n, csr, csc)
    return (count, labels, sizes, stats) if with_stats else (count, labels, sizes)


def graph_color_refinement(graph, initial=None, order=None, max_rounds=None, hash_mask: int = -1, timed: bool = False):
    """``(colours int64 [n] on the compute device, _hip.WlStats)`` of one graph's CSR (csrc/pp_graph_wl.hip).  A CPU-resident graph, and a
    CPU ``initial`` / ``order``, are staged, as in :func:`graph_components`."""
    dev = compute_device(graph.data.edge_index)
    row_ptr, col, initial, order = _stage(dev, graph.row_ptr, graph.col, initial, order)
    return _hip.graph_wl_refine(row_ptr, col, graph.n, initial, order, max_rounds, hash_mask, timed)


def graph_pair_color_refinement(g1, g2, initial=None, order=None, hash_mask: int = -1):
    """The same on the disjoint union of two graphs: the block-diagonal concatenation of their CSRs on the compute device (the nodes of
    ``g2`` follow those of ``g1``; no ID is touched, no edge list is rebuilt)."""
    dev = compute_device(g1.data.edge_index, g2.data.edge_index)
    ptr1, col1, ptr2, col2, initial, order = _stage(dev, g1.row_ptr, g1.col, g2.row_ptr, g2.col, initial, order)
    row_ptr = torch.cat((ptr1[:-1], ptr2 + col1.numel()))
    col = torch.cat((col1, col2 + g1.n))
    return _hip.graph_wl_refine(row_ptr, col, g1.n + g2.n, initial, order, None, hash_mask)


POWER_EIGENVECTOR, POWER_KATZ = _hip.POWER_EIGENVECTOR, _hip.POWER_KATZ


def graph_entry_weights(graph, attr: str, dev) -> torch.Tensor:
    """float64 ``[k]`` on ``dev``: the edge attribute ``attr`` summed over the parallel edges behind every entry of
    ``graph.simple_successors()``, in that structure's order."""
    values = torch.as_tensor(graph.data[attr]).reshape(-1).to(dev).to(torch.float64)
    if graph.simple_successors()[3] is None:                            # (the stored list is its own simple structure)
        return values
    (ei,) = _stage(dev, graph.data.edge_index)
    return _hip.coalesce(ei, values, graph.n, "sum")[1]


def graph_power_centrality(graph, mode: int, threshold: float, max_iter: int, alpha: float = 0.0, beta=0.0, start=None,
                           normalized: bool = True, weight: str | None = None, group: int = 0, heavy_min: int = 0, batch: int = 0,
                           with_stats: bool = False):
    """``(values float64 [n] on the compute device, iterations, converged)`` of the power iteration ``mode`` (``_hip.POWER_EIGENVECTOR`` /
    ``_hip.POWER_KATZ``; csrc/pp_graph_power.hip) over ``graph.simple_predecessors()``; with ``with_stats`` the ``_hip.PowerStats`` follow.
    ``weight`` names an edge attribute (summed over parallel edges) or is ``None`` (every distinct edge counts 1); ``beta`` is a number or
    a float64 ``[n]`` tensor, ``start`` a float64 ``[n]`` tensor or ``None``.  ``group``, ``heavy_min``, ``batch``: 0 = the library's
    choice; they never change which iterate is returned.  A CPU-resident graph and CPU vectors are staged, as in :func:`graph_components`."""
    dev = compute_device(graph.data.edge_index)
    col_ptr, row, perm = _stage(dev, *graph.simple_predecessors())
    w = None if weight is None else graph_entry_weights(graph, weight, dev)[perm]
    beta, start = (t.to(dev).to(torch.float64) if isinstance(t, torch.Tensor) else t for t in (beta, start))
    values, stats = _hip.graph_power_iterate(col_ptr, row, w, graph.n, mode, threshold, max_iter, alpha, beta, start, normalized, group,
                                             heavy_min, batch)
    return (values, stats.iterations, stats.converged, stats) if with_stats else (values, stats.iterations, stats.converged)


DIFFUSION_PAGERANK, DIFFUSION_WALK = _hip.DIFFUSION_PAGERANK, _hip.DIFFUSION_WALK


def graph_diffusion_structure(graph, weight: str | None = None, count_stored: bool = False):
    """``(col_ptr, src, _hip.DiffusionTable)`` on the compute device: the pull structure of ``graph.simple_predecessors()`` with the transition
    probabilities of csrc/pp_graph_diffusion.hip.  An entry weighs the edge attribute ``weight`` summed over its parallel edges, or with
    ``weight=None`` the number of stored edges behind it (``count_stored``: the view of ``RandomWalk``) or 1 (networkx's view).  The caller
    looks at ``table.bad``.  A CPU-resident graph is staged, as in :func:`graph_components`."""
    dev = compute_device(graph.data.edge_index)
    row_ptr, _, _, mult = _graph_simple(graph, dev)
    col_ptr, src, perm = _stage(dev, *graph.simple_predecessors())
    if weight is not None:
        w = graph_entry_weights(graph, weight, dev)
    else:
        w = mult.to(torch.float64) if count_stored and mult is not None else None
    return col_ptr, src, _hip.diffusion_table(row_ptr, w, src, perm, graph.n)


def graph_diffusion(structure, n: int, mode: int, start, threshold: float, max_iter: int, alpha: float = 0.0, lazy: float = 0.0, p=None, d=None,
                    target=None, keep_all: bool = False, want_tvd: bool = False, batch: int = 0, heavy_min: int = 0):
    """``_hip.DiffusionRun`` of the propagator over ``structure`` (:func:`graph_diffusion_structure`) from the float64 ``[n, B]`` block
    ``start``; ``p`` and ``d`` (PageRank) have its shape, ``target`` is ``[n]``.  More than 64 columns run in tiles of 64 and are put
    together: a column's bits do not depend on its tile.  ``batch``, ``heavy_min``: 0 = the library's choice.  CPU blocks are staged."""
    col_ptr, src, table = structure
    dev = col_ptr.device
    same = d is p
    start, p, d, target = (None if t is None else torch.as_tensor(t).to(dev).to(torch.float64) for t in (start, p, d, target))
    if same:
        d = p
    B, tile = int(start.size(1)), _hip.DIFFUSION_MAX_WIDTH
    runs = []
    for c0 in range(0, B, tile):
        cols = slice(c0, min(c0 + tile, B))
        p_t = None if p is None else p[:, cols]
        d_t = p_t if same else (None if d is None else d[:, cols])
        runs.append(_hip.diffusion_run(col_ptr, src, table, n, mode, start[:, cols], threshold, max_iter, alpha, lazy, p_t, d_t, target,
                                       keep_all, want_tvd, batch, heavy_min))
    if len(runs) == 1:
        return runs[0]
    return _hip.DiffusionRun(torch.cat([r.final for r in runs], 1), sum((r.iterations for r in runs), []), sum((r.converged for r in runs), []),
                             torch.cat([r.trajectory for r in runs], 2) if keep_all else None,
                             torch.cat([r.tvd for r in runs], 1) if want_tvd else None, runs[0].grids)


def diffusion_project(ptr, idx, rows: int, x, heavy_min: int = 0):
    """float64 ``[rows, B]``: the rows ``idx[ptr[r] : ptr[r + 1]]`` of ``x`` (float64 ``[n, B]``) summed per group, in tiles of 64 columns."""
    dev = compute_device(ptr, idx, x)
    ptr, idx, x = _stage(dev, ptr, idx, x)
    tile = _hip.DIFFUSION_MAX_WIDTH
    outs = [_hip.diffusion_project(ptr, idx, rows, x[:, c0:c0 + tile], heavy_min) for c0 in range(0, int(x.size(1)), tile)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, 1)


def layout_adjacency(edge_index, weight, num_nodes: int):
    """``(ptr, nbr, w)`` on the compute device: the symmetric adjacency the reference's layouts see (csrc/pp_graph_layout.hip) — one entry
    per unordered pair with a stored edge in either direction, valued 1 or, with ``weight`` (one value per stored edge), by the LAST such
    edge in stored order; self-loops dropped.  CPU-resident inputs are staged."""
    dev = compute_device(edge_index, weight)
    ei, weight = _stage(dev, edge_index, weight)
    return _hip.graph_layout_adjacency(ei, weight, num_nodes)


def graph_layout_adjacency(graph, weight=None):
    """:func:`layout_adjacency` of a Graph; ``weight``: ``None``, the name of an edge attribute or a tensor with one value per stored edge."""
    if isinstance(weight, str):
        weight = torch.as_tensor(graph.data[weight])
    return layout_adjacency(graph.data.edge_index, weight, graph.n)


def graph_fr_layout(adjacency, pos, k: float, t, dt, iterations: int, threshold: float, fixed=None, with_stats: bool = False, block: int = 0,
                    chunks: int = 0, group: int = 0, heavy_min: int = 0, batch: int = 0):
    """``(pos float64 [n, 2] on the compute device, iterations_run, last_err)`` of the Fruchterman-Reingold iteration (csrc/pp_graph_layout.hip)
    from ``pos`` over ``adjacency = (ptr, nbr, w)``; with ``with_stats`` the ``_hip.LayoutStats`` follow.  ``t`` and ``dt``: the temperature
    and its step, or ``t=None`` for networkx's (a tenth of the larger extent of ``pos``, ``t / (iterations + 1)``), computed on the
    device.  ``fixed``: a bool / uint8 ``[n]`` mask or ``None``.  Kernel settings, 0 = the library's choice: ``block`` (targets per
    repulsion workgroup: 64, 128, 256), ``chunks`` (pieces of the source range, up to 64), ``group`` (lanes per neighbour list),
    ``heavy_min`` (list length that gets a whole workgroup), ``batch`` (iterations per read-back; never changes a bit).  CPU-resident
    inputs are staged."""
    dev = compute_device(pos, *adjacency)
    ptr, nbr, w, pos, fixed = _stage(dev, *adjacency, torch.as_tensor(pos), None if fixed is None else torch.as_tensor(fixed))
    out, ran, err, stats = _hip.graph_layout_iterate(ptr, nbr, w, pos.to(torch.float64), k, t, dt, iterations, threshold, fixed, block, chunks,
                                                     group, heavy_min, batch)
    return (out, ran, err, stats) if with_stats else (out, ran, err)


def layout_start(seed: int, n: int, dom_size: float, center, given=None, has=None, device=None):
    """Start positions of the spring layout on the compute device: ``given`` (float64 ``[n, 2]``) where ``has`` (bool ``[n]``; ``None``:
    everywhere), else Philox draws ``uniform[0, 1) * dom_size + center``."""
    dev = random_device(device)
    given, has = _stage(dev, given, has)
    if given is not None:
        given = given.to(torch.float64).contiguous()
    if has is not None:
        has = has.to(torch.uint8).contiguous()
    return _hip.graph_layout_start(seed, n, dom_size, center, given, has, dev)


def layout_random(seed: int, n: int, center, device=None):
    return _hip.graph_layout_random(seed, n, center, random_device(device))


def layout_closed_form(kind: int, n: int, device=None):
    return _hip.graph_layout_closed_form(kind, n, random_device(device))


def layout_rescale(pos, scale: float, center):
    return _hip.graph_layout_rescale(pos, scale, center)


LAYOUT_CIRCULAR, LAYOUT_GRID = _hip.LAYOUT_CIRCULAR, _hip.LAYOUT_GRID


def random_device(device=None) -> torch.device:
    """Where a random graph is sampled: ``device`` if it names a GPU, else the current one (a host ``device`` only receives the result)."""
    if device is not None and torch.device(device).type == "cuda":
        compute_device()
        d = torch.device(device)
        return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())
    return compute_device()


def random_regions(rows: list, n_chunks: int, seed: int, n: int, device=None, perm=None):
    """The edges (int64 ``[2, E]`` on the compute device) of the region descriptors ``rows`` (host lists; csrc/pp_random_graphs.hip)."""
    dev = random_device(device)
    table = torch.tensor(rows, dtype=torch.int64).reshape(-1, 8).to(dev)
    (perm,) = _stage(dev, perm)
    return _hip.rg_regions_sample(table, n_chunks, seed, n, perm)


def random_block_order(z, num_blocks: int, device=None):
    """``(sizes, perm)`` of a block assignment (staged if it is CPU-resident): the block sizes as a host list and the stable order of the
    nodes by block (rank -> node) on the compute device."""
    dev = random_device(device)
    (z,) = _stage(dev, z)
    return _hip.degree(z, num_blocks).tolist(), _hip.argsort(z, (0, max(num_blocks - 1, 0)))


def random_draws(below: int, seed: int, first: int, count: int, device=None, tag: int = _hip.RG_TAG_GNM):
    return _hip.rg_draws(below, seed, first, count, random_device(device), tag)


def random_first_distinct(values, m: int, bits: int):
    return _hip.rg_first_distinct(values, m, bits)


def random_sorted(values, bits: int):
    return _hip.sort_pairs(values, None, 0, max(bits, 1))[0] if values.numel() > 1 else values


def random_complement(excluded, total: int, device=None):
    if excluded is None:
        excluded = torch.empty(0, dtype=torch.int64, device=random_device(device))
    return _hip.rg_complement(excluded, total)


def random_decode(slots, kind: int, cols: int):
    dev = compute_device(slots)
    (slots,) = _stage(dev, slots)
    return _hip.rg_decode(slots, kind, cols)


def random_sort_edges(edge_index, n: int):
    return _hip.rg_sort_edges(edge_index, n)


def random_ring(n: int, s: int, seed: int, threshold: int, always: bool, undirected: bool, no_dups: bool, no_loops: bool, max_rounds: int,
                device=None):
    """The rewired ring lattice (int64 ``[2, n s]``, unsorted) after as many repair rounds as it takes (one read-back per round)."""
    edge_index = _hip.rg_ws_edges(n, s, seed, threshold, always, undirected, random_device(device))
    if no_dups or no_loops:
        for rnd in range(1, max_rounds + 1):
            if _hip.rg_ws_repair(edge_index, n, seed, rnd, no_dups, no_loops, undirected) == 0:
                return edge_index
        raise RuntimeError(f"watts_strogatz: edges are still to be repaired after {max_rounds} rounds")
    return edge_index


def random_degrees(degrees, device=None):
    """An int64 degree vector on the compute device (a CPU-resident one is staged, like ``z`` of the block model)."""
    dev = degrees.device if degrees.is_cuda else random_device(device)
    (degrees,) = _stage(dev, degrees)
    return degrees.to(torch.int64).contiguous()


def random_graphic(degrees) -> bool:
    """The Erdös-Gallai test of an int64 degree vector on the compute device: the range from ``minmax`` (a degree is in 0 .. n - 1), parity
    and the condition for r = 1 .. n from ``k_eg_check``."""
    n = degrees.numel()
    if n == 0:
        return True
    lo, hi = _hip.minmax(degrees)
    if lo < 0 or hi > n - 1:
        return False
    return _hip.rg_eg_check(degrees)


def random_matching(degrees, n: int, seed: int, multi: bool, relax: bool, max_rounds: int):
    """``(edges, rounds)`` of the Molloy-Reed sampler: int64 ``[2, S / 2]`` on the device of ``degrees`` (unsorted, ends sorted) after as many
    repair rounds as it takes (one read-back per round; none with ``relax``), or ``(None, 0)`` for S = 0."""
    ptr = _hip.exclusive_scan(degrees)
    stubs = int(ptr[-1].item())
    if stubs >= 0x7fffffff:
        raise ValueError(f"molloy_reed: the degrees sum to {stubs}, 2^31 - 1 or more (stub and edge indices are int32 in the sort)")
    if stubs == 0:
        return None, 0
    edge_index = _hip.rg_mr_matching(ptr, n, stubs, seed)
    if relax:
        return edge_index, 0
    for rnd in range(1, max_rounds + 1):
        if _hip.rg_mr_repair(edge_index, n, seed, rnd, multi) == 0:
            return edge_index, rnd - 1
    raise RuntimeError(f"molloy_reed: edges are still to be repaired after {max_rounds} rounds")


def count_unordered(edge_index) -> int:
    if edge_index.size(1) < 2:
        return 0
    dev = compute_device(edge_index)
    (ei,) = _stage(dev, edge_index)
    return _hip.count_unordered(ei)


def _graph_simple(graph, dev):
    """The simple successor structure of a Graph (wherever it lives) on the compute device: ``(row_ptr, row, col, mult | None)``."""
    return _stage(dev, *graph.simple_successors())


def graph_triad_counts(graph):
    """The number of closed triads of every node: int64 ``[n]`` on the compute device (csrc/pp_graph_triads.hip).  A CPU-resident graph
    is staged, as in :func:`graph_components`."""
    dev = compute_device(graph.data.edge_index)
    row_ptr, row, col, _ = _graph_simple(graph, dev)
    return _hip.graph_triad_node_counts(row_ptr, row, col, graph.n)


def graph_triads_of(graph, v: int, want_pairs: bool):
    """Node ``v`` alone: ``(count, pairs)`` with the closed triads as int64 ``[2, count]`` index pairs on the compute device (``None``
    unless wanted) — the entry counts of v's row, their scan, the fill."""
    dev = compute_device(graph.data.edge_index)
    row_ptr, row, col, _ = _graph_simple(graph, dev)
    e0, e1 = row_ptr[v:v + 2].tolist()
    scan = _hip.exclusive_scan(_hip.graph_triad_entry_counts(row_ptr, row, col, graph.n, e0, e1))
    total = int(scan[-1].item())
    return total, (_hip.graph_triad_fill(row_ptr, col, graph.n, v, scan, total) if want_pairs else None)


def graph_pair_meets(graph, pairs, table=None, want_dot: bool = False, want_sizes: bool = False):
    """``(common, dot | None, aa | None, sizes | None)`` of the index pairs ``pairs`` [2, P] on the compute device; ``table``: a host float64 array indexed
    by stored out-degree, which switches ``aa`` on."""
    dev = compute_device(graph.data.edge_index)
    row_ptr, _, col, mult = _graph_simple(graph, dev)
    (pairs,) = _stage(dev, pairs)
    deg_ptr = None
    if table is not None:
        (deg_ptr,) = _stage(dev, graph.row_ptr)
        table = torch.as_tensor(table, dtype=torch.float64).to(dev)
    return _hip.graph_pair_meets(row_ptr, col, mult, graph.n, pairs, deg_ptr, table, want_dot, want_sizes)


def degree_product_sum(graph, a, b) -> int:
    dev = compute_device(graph.data.edge_index)
    ei, a, b = _stage(dev, graph.data.edge_index, a, b)
    return _hip.degree_product_sum(ei, graph.n, a, b)


def graph_clustering(graph, triads, want_coeff: bool, want_mean: bool):
    """Local coefficients (float64 ``[n]``) and / or the mean of their float32 roundings (float64 ``[1]``) on the compute device, from the
    degree the reference normalises with: stored out-degrees, stored in-degrees for a graph flagged undirected."""
    dev = compute_device(graph.data.edge_index)
    deg = graph.degrees(mode="in" if graph.is_undirected() else "out", return_tensor=True)
    triads, deg = _stage(dev, triads, deg)
    return _hip.graph_clustering(triads, deg, want_coeff, want_mean)


def degree_histogram(graph, degree_seq):
    """``bincount`` of a degree sequence as a kernel (``pp_degree_i64``): int32 ``[max degree + 1]`` on the compute device."""
    dev = compute_device(graph.data.edge_index)
    (seq,) = _stage(dev, degree_seq)
    seq = seq.to(torch.int64)
    if seq.numel() == 0:
        return torch.empty(0, dtype=torch.int32, device=dev)
    return _hip.degree(seq, _hip.minmax(seq)[1] + 1)


def linegraph_lift(edge_index, num_nodes: int, edge_range=None):
    dev = compute_device(edge_index)
    (ei,) = _stage(dev, edge_index)
    return _back(edge_index, _hip.linegraph_lift(ei, num_nodes, edge_range))


def edge_attr(edge_index, attr, aggr: str):
    dev = compute_device(edge_index, attr)
    ei, a = _stage(dev, edge_index, attr)
    return _back(edge_index, _hip.edge_attr(ei, a, aggr))


def extend_node_sequence(edge_index, node_sequence):
    dev = compute_device(edge_index, node_sequence)
    ei, ns = _stage(dev, edge_index, node_sequence)
    return _back(edge_index, _hip.extend_node_sequence(ei, ns))


def gather_concat(rows, idx, suffix):
    dev = compute_device(rows, idx, suffix)
    r, i, sfx = _stage(dev, rows, idx, suffix)
    return _back(rows, _hip.gather_concat(r, i, sfx))


def unique_rows(rows, value_range=None):
    dev = compute_device(rows)
    (r,) = _stage(dev, rows)
    return _back(rows, *_hip.unique_rows(r, value_range))


def coalesce(edge_index, weight, num_nodes: int, reduce: str = "sum", remap=None, want_inverse: bool = False, col_block=None):
    dev = compute_device(edge_index, None if isinstance(weight, str) else weight, remap)
    ei, w, rm = _stage(dev, edge_index, weight, remap)
    if col_block is not None:
        col_block = (_stage(dev, col_block[0])[0], col_block[1])
    return _back(edge_index, *_hip.coalesce(ei, w, num_nodes, reduce, rm, want_inverse, col_block))


def successor_blocks(block_key, num_blocks: int, node_block):
    """Column blocks for :func:`coalesce` on a De Bruijn layer: the nodes are numbered lexicographically, ``block_key[u]`` (sorted,
    non-decreasing) is the id of node u's prefix and ``node_block[u]`` the prefix id that every SUCCESSOR of u shares.  Returns
    ``(col_base [U], col_bits)``: successors of u have ids in ``[col_base[u], col_base[u] + 2**col_bits)``."""
    dev = compute_device(block_key, node_block)
    key, blk = _stage(dev, block_key, node_block)
    ptr = _hip.ptr_from_sorted(key, num_blocks)
    widest = int((ptr[1:] - ptr[:-1]).max().item()) if num_blocks > 0 else 1
    bits = max(int(widest - 1).bit_length(), 1)
    return ptr[blk], bits


def minmax(a):
    dev = compute_device(a)
    (x,) = _stage(dev, a)
    return _hip.minmax(x)


def is_sorted(a) -> bool:
    if a.numel() < 2:
        return True
    dev = compute_device(a)
    (x,) = _stage(dev, a)
    return _hip.is_sorted(x)


def time_stats(time):
    dev = compute_device(time)
    (t,) = _stage(dev, time)
    return _hip.time_stats(t)


def gather_events(edge_index, time, perm):
    dev = compute_device(edge_index, time, perm)
    ei, t, p = _stage(dev, edge_index, time, perm)
    return _back(edge_index, *_hip.gather_events(ei, t, p))


def stable_argsort(keys, value_range=None):
    dev = compute_device(keys)
    (k,) = _stage(dev, keys)
    return _back(keys, _hip.argsort(k, value_range))


def ptr_from_sorted(sorted_index, num_rows: int):
    dev = compute_device(sorted_index)
    (s,) = _stage(dev, sorted_index)
    return _back(sorted_index, _hip.ptr_from_sorted(s, num_rows))
