"""PageRank on the GPU: :func:`pagerank` (``networkx.pagerank`` 3.4 on the distinct stored edges) and :func:`personalized_pagerank`, many
personalisations at once, on the batched propagator of ``csrc/pp_graph_diffusion.hip`` (the header's "distributions and PageRank" block).

Both are exported from :mod:`pathpyg_amd.algorithms`.  They live here and not in :mod:`~pathpyg_amd.algorithms.centrality`: that module
mirrors the reference's, whose ``__getattr__`` forwards unknown names to ``networkx.algorithms.centrality`` — where ``pagerank`` is not (it
is ``networkx.algorithms.link_analysis``) — so ``centrality.pagerank`` stays the ``AttributeError`` it is in the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _dispatch, _hip
from .centrality import PowerIterationFailedConvergence, _check_power_arguments, _node_vector, _power_result


def _checked_weights(v: torch.Tensor, name: str) -> torch.Tensor:
    if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
        raise ValueError(f"{name} must be finite and not negative")
    return v


def _distribution_vector(value, n: int, name: str) -> torch.Tensor:
    """``value`` in the forms of :func:`_node_vector` as a checked float64 ``[n]`` tensor on the host, not yet normalised.  A dict may be
    partial, as in networkx: missing indices are 0; a key that is no node index is refused."""
    if isinstance(value, dict):
        v = torch.zeros(n, dtype=torch.float64)
        for key, x in value.items():
            if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < n:
                raise ValueError(f"{name}: {key!r} is no node index in [0, {n})")
            v[int(key)] = float(x)
    else:
        v = _node_vector(value, n, name).cpu()
    return _checked_weights(v, name)


def normalized_columns(block: torch.Tensor, name: str) -> torch.Tensor:
    """Every column of the float64 ``[n, B]`` host block divided by its sum, each from its own contiguous copy: a column gets the same bits
    whichever block it comes in.  ``ValueError`` for a column that sums to 0."""
    out = torch.empty(tuple(block.shape), dtype=torch.float64)
    for c in range(block.size(1)):
        col = block[:, c].contiguous()
        total = col.sum()
        if not float(total) > 0.0:
            raise ValueError(f"{name} cannot have all zero values" + (f" (column {c})" if block.size(1) > 1 else ""))
        out[:, c] = col / total
    return out


def _pagerank_block(graph, alpha: float, start, p, d, max_iter: int, tol: float, weight):
    """The ``_hip.DiffusionRun`` of PageRank from the ``[n, B]`` blocks ``start``, ``p``, ``d`` (``d is p``: the default dangling weights)."""
    structure = _dispatch.graph_diffusion_structure(graph, weight)
    if structure[2].bad:
        raise ValueError(f"edge attribute {weight!r}: PageRank needs finite weights that are not negative")
    return _dispatch.graph_diffusion(structure, graph.n, _dispatch.DIFFUSION_PAGERANK, start, graph.n * tol, int(max_iter), alpha=alpha, p=p, d=d)


def _check_pagerank_arguments(graph, alpha, max_iter, weight, columns: int) -> float:
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
    _check_power_arguments(graph, max_iter, weight)
    _hip.diffusion_check_sizes(graph.n, int(graph.data.peek("edge_index").shape[1]), _hip.diffusion_width(min(max(columns, 1), _hip.DIFFUSION_MAX_WIDTH)), 2)
    return alpha


def pagerank(graph, alpha: float = 0.85, personalization=None, max_iter: int = 100, tol: float = 1e-06, nstart=None, weight: str | None = None,
             dangling=None, *, return_tensor: bool = False):
    """PageRank as ``networkx.pagerank`` (3.4) computes it on the copy the reference would make — a DiGraph of the DISTINCT stored edges,
    self-loops kept: from ``x = nstart / sum(nstart)`` (default ``1 / n``) every iteration is
    ``x' = alpha * (x A + D * dangling) + (1 - alpha) * personalization`` with ``A[u, v] = w(u, v) / T_u``, ``T_u`` the weight sum of u's
    out-entries, ``D`` the sum of ``x`` over the dangling nodes (``T_u = 0``); ``personalization`` and ``dangling`` are normalised to sum 1
    (defaults: ``1 / n``, and the personalisation).  It stops at the first iterate with ``sum |x' - x| < n * tol``.  networkx's arguments,
    order and defaults.

    ``weight=None`` counts every distinct edge as 1; a string names an edge attribute, summed over parallel edges (the extension of
    :func:`eigenvector_centrality`).  The vectors take the forms of ``nstart`` there; a dict may be partial, as in networkx (missing node
    indices are 0).  Deviations from networkx, all refusals: ``ValueError`` for a negative or non-finite entry, an all-zero vector (networkx:
    ``ZeroDivisionError``), a dict key that is no node index, ``alpha`` outside [0, 1] and weights that are negative or not finite (networkx
    runs on into NaN).

    Returns ``{node id: float}`` in index order or, with ``return_tensor=True``, the float64 ``[n]`` tensor on the compute device; ``{}``
    (an empty tensor) for the null graph.  Raises :class:`PowerIterationFailedConvergence` after ``max_iter`` iterations without
    convergence.  Everything runs on the GPU (csrc/pp_graph_diffusion.hip); the result has the same bits on every run."""
    n = graph.n
    alpha = _check_pagerank_arguments(graph, alpha, max_iter, weight, 1)
    if n == 0:
        return torch.empty(0, dtype=torch.float64, device=graph.device) if return_tensor else {}
    vectors = {name: None if v is None else normalized_columns(_distribution_vector(v, n, name).reshape(-1, 1), name)
               for name, v in (("nstart", nstart), ("personalization", personalization), ("dangling", dangling))}
    uniform = torch.full((n, 1), 1.0 / n, dtype=torch.float64)
    start = uniform if vectors["nstart"] is None else vectors["nstart"]
    p = uniform if vectors["personalization"] is None else vectors["personalization"]
    d = p if vectors["dangling"] is None else vectors["dangling"]
    run = _pagerank_block(graph, alpha, start, p, d, max_iter, tol, weight)
    return _power_result(graph, run.final.reshape(-1), run.converged[0], max_iter, return_tensor)


def personalized_pagerank(graph, seeds, alpha: float = 0.85, max_iter: int = 100, tol: float = 1e-06, weight: str | None = None) -> torch.Tensor:
    """:func:`pagerank` for many personalisations at once: the float64 ``[n, B]`` tensor on the compute device whose column ``c`` equals
    ``pagerank(graph, alpha, personalization=column c, ...)`` bit for bit — the B distributions of a node are B contiguous doubles, and a
    column's arithmetic does not depend on the others (more than 64 columns run in tiles of 64).  A column that has met the criterion keeps
    that iterate while the others go on.

    ``seeds``: a list of node IDs or an integer tensor of node INDICES ``[B]`` (one one-hot personalisation each), or a float ``[n, B]``
    matrix of personalisations (normalised per column).  Start ``1 / n``, dangling weights = the personalisation.  Raises
    :class:`PowerIterationFailedConvergence` if any column has not converged after ``max_iter`` iterations; its ``columns`` lists them."""
    n = graph.n
    matrix = None
    if isinstance(seeds, (torch.Tensor, np.ndarray)) and torch.as_tensor(seeds).dtype.is_floating_point:
        matrix = torch.as_tensor(seeds).to(torch.float64).cpu()
        if matrix.dim() != 2 or matrix.size(0) != n:
            raise ValueError(f"a personalisation matrix must be [n = {n}, B], got {tuple(matrix.shape)}")
        B = int(matrix.size(1))
    else:
        if isinstance(seeds, (torch.Tensor, np.ndarray)):
            idx = torch.as_tensor(seeds)
            if idx.dtype == torch.bool or idx.dim() != 1:
                raise ValueError("seeds: a list of node ids, a one-dimensional tensor of node indices or a float [n, B] matrix")
            idx = idx.to(torch.int64).cpu()
        elif isinstance(seeds, (list, tuple)):
            try:
                idx = torch.tensor([int(graph.mapping.to_idx(s)) for s in seeds], dtype=torch.int64)
            except KeyError as e:
                raise ValueError(f"seeds: unknown node id {e}") from None
        else:
            raise ValueError("seeds: a list of node ids, a one-dimensional tensor of node indices or a float [n, B] matrix")
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f"seeds: node index outside [0, {n})")
        B = int(idx.numel())
    alpha = _check_pagerank_arguments(graph, alpha, max_iter, weight, B)
    if matrix is not None:
        p = normalized_columns(_checked_weights(matrix, "seeds"), "seeds")
    dev = _dispatch.compute_device(graph.data.edge_index)
    if n == 0 or B == 0:
        return torch.empty((n, B), dtype=torch.float64, device=dev)
    if matrix is None:
        p = torch.zeros((n, B), dtype=torch.float64, device=dev)
        p[idx.to(dev), torch.arange(B, device=dev)] = 1.0
    start = torch.full((n, B), 1.0 / n, dtype=torch.float64, device=dev)
    run = _pagerank_block(graph, alpha, start, p, p, max_iter, tol, weight)
    failed = [c for c, ok in enumerate(run.converged) if not ok]
    if failed:
        raise PowerIterationFailedConvergence(max_iter, failed)
    return run.final
