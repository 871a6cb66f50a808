"""Node layouts, HIP-backed (reference ``pathpyG.visualisations.layout``): the coordinates every plot of the reference starts from.

```py
import pathpyg_amd as pp

g = pp.Graph.from_edge_list([("a", "b"), ("b", "c"), ("c", "a"), ("c", "d")])
pos = pp.layout(g, "spring", seed=1)                              # {node id: ndarray [2]}
xy = pp.layout(g, "fr", k=0.3, iterations=100, return_tensor=True)   # float64 [n, 2] on the GPU, index order
```

:func:`layout` and :class:`Layout` keep the reference's signatures.  The reference converts the graph to networkx and calls its layout
functions; this package has no networkx dependency and no CPU path, so the layouts that are arithmetic run as kernels
(csrc/pp_graph_layout.hip) and the rest is refused:

* **spring** (``spring``, ``fr``, ``fruchterman-reingold``, ``fruchterman_reingold``, ``spring_layout``, ``spring layout``):
  ``networkx.spring_layout`` of networkx 3.4, with its arguments in its order and with its defaults: ``k=None, pos=None, fixed=None,
  iterations=50, threshold=1e-4, scale=1, center=None, dim=2, seed=None``.  ``pos`` is a dict keyed by node id (it may cover some nodes
  only) or an ``[n, 2]`` array in index order; nodes without a position are drawn as ``uniform[0, 1) * dom_size + center``, ``dom_size``
  being the largest given coordinate (1 if that is 0); with ``pos=None`` every node is drawn in ``[0, 1)``.  ``fixed`` lists node ids that
  keep their position; each needs one.  ``k`` defaults to ``1 / sqrt(n)``, or to ``dom_size / sqrt(n)`` when ``fixed`` is given.  The result
  is rescaled (mean to ``center``, largest ``|coordinate|`` to ``scale``) unless ``fixed`` is given or ``scale`` is ``None``.  ``dim``
  must be 2.  The iteration runs until ``sqrt(sum |dp|^2) / n < threshold`` or ``iterations`` times; :data:`last_iterations` keeps the count.

  The adjacency is the one the reference builds: symmetric, one entry per unordered pair of distinct nodes with a stored edge in either
  direction; with ``weight`` its value is the weight of the LAST such edge in stored order (a later ``add_edge`` overwrites an earlier one).
  Self-loops exert no force.  Zero and negative weights mean what the arithmetic says.

  **Departure from networkx.**  From 500 nodes on networkx switches to a float32 loop over rows; its float32 and float64 runs of the same
  graph differ by 10 - 50 % of the layout's size after 50 iterations.  Here the float64 form — the one networkx uses below 500 nodes —
  runs at every n.  The map is chaotic (a rounding difference grows about threefold per iteration), so a 50-iteration layout agrees with
  networkx's in kind, not in digits; single steps and short runs agree to rounding ("Node layouts").
* **random** (``random``, ``rand``, ``None``): float32 in ``[0, 1) + center``, arguments ``center=None, dim=2, seed=None``.
* **circular** (``circular``, ``circle``, ``ring``, ``1d-lattice``, ``lattice-1d``): networkx's angles ``2 pi i / n`` in float32, its rescale
  and ``center``; arguments ``scale=1, center=None, dim=2``.
* **grid** (``grid``, ``2d-lattice``, ``lattice-2d``): the reference's own formula.
* shell, spectral, Kamada-Kawai and ForceAtlas2 are **not ported** (they need an eigen-solver, L-BFGS or a second force model): a
  ``NotImplementedError`` names the layout.  Any other string raises the reference's ``ValueError``.

**Random draws are not networkx's.**  networkx draws from a numpy ``RandomState``; here a draw is a word of the package's Philox4x32-10
stream (tag ``PP_RG_TAG_LAYOUT``, index ``2 * node + axis``) — a pure function of ``seed``, following the ``seed`` convention of
:mod:`pathpyg_amd.algorithms.generative_models`: an int of any sign counts modulo 2^64, ``None`` draws one from torch's default CPU
generator (so ``torch.manual_seed`` makes a script reproducible) and the seed used is kept in ``generative_models.last_seed``.  The same
seed gives the same coordinates, bit for bit, on every run; numpy's stream for that seed is not reproduced.

As an extension every entry point takes the keyword-only ``return_tensor=True`` and then returns the ``[n, 2]`` tensor on the compute
device, in index order, instead of the dictionary (which is read back once).
"""
from __future__ import annotations

import math
from collections.abc import Iterable
from typing import Optional

import numpy as np
import torch

from .. import _dispatch
from ..algorithms.generative_models import _seed

NAMES_GRID = ("grid", "2d-lattice", "lattice-2d")
NAMES_RANDOM = ("random", "rand", None)
NAMES_CIRCULAR = ("circular", "circle", "ring", "1d-lattice", "lattice-1d")
NAMES_SPRING = ("fruchterman-reingold", "fruchterman_reingold", "fr", "spring_layout", "spring layout", "spring")
NAMES_NOT_PORTED = {
    "shell": ("shell", "concentric", "concentric-circles", "shell layout"),
    "spectral": ("spectral", "eigen", "spectral layout"),
    "kamada-kawai": ("kamada-kawai", "kamada_kawai", "kk", "kamada", "kamada layout"),
    "forceatlas2": ("forceatlas2", "fa2", "forceatlas", "force-atlas", "force-atlas2", "fa 2"),
}

last_iterations = None       # iterations the most recent spring layout ran
last_err = None              # its last sqrt(sum |dp|^2) / n


def layout_family(name) -> str:
    """``"grid" | "random" | "circular" | "spring"`` of a lower-cased layout name; ``NotImplementedError`` for the layouts that are not
    ported, the reference's ``ValueError`` for every other name."""
    if name in NAMES_GRID:
        return "grid"
    if name in NAMES_RANDOM:
        return "random"
    if name in NAMES_CIRCULAR:
        return "circular"
    if name in NAMES_SPRING:
        return "spring"
    for family, names in NAMES_NOT_PORTED.items():
        if name in names:
            raise NotImplementedError(f"Layout '{name}' ({family}) is not ported: pathpyg_amd computes the spring, random, circular and grid "
                                      "layouts on the GPU and has no networkx fallback")
    raise ValueError(f"Layout '{name}' not recognized.")


def layout(network, layout: str = "random", weight: None | str | Iterable = None, *, return_tensor: bool = False, **kwargs):
    """Node positions of ``network`` under the layout ``layout`` (reference layout.py:69-132): ``{node id: ndarray [2]}`` in index order.

    ``weight``: the name of an edge attribute, an iterable or a tensor with one value per stored edge, or ``None``.  ``kwargs`` go to the
    layout (see the module docstring).  Raises ``ValueError`` for an unknown weight attribute, for an iterable of the wrong length and for
    an unknown layout name; ``NotImplementedError`` for a layout that is not ported."""
    if isinstance(weight, str):
        if weight in network.edge_attrs():
            weight = network.data[weight]
        else:
            raise ValueError(f"Weight attribute '{weight}' not found in edge attributes.")
    elif isinstance(weight, Iterable) and not isinstance(weight, torch.Tensor):
        n_edges = network.m * 2 if network.is_undirected() else network.m
        if len(weight) == n_edges:  # type: ignore[arg-type]
            weight = torch.tensor(weight)
        else:
            raise ValueError("Length of weight iterable does not match number of edges in the network.")
    return Layout(nodes=network.nodes, edge_index=network.data.edge_index, layout_type=layout, weight=weight, return_tensor=return_tensor,
                  **kwargs).generate_layout()


def _center(center, dim) -> np.ndarray:
    if dim != 2:
        raise ValueError(f"dim must be 2, got {dim}: pathpyg_amd computes planar layouts only (the reference's plots are 2-D)")
    center = np.zeros(2) if center is None else np.asarray(center, dtype=np.float64)
    if center.shape != (2,):
        raise ValueError("length of center coordinates must match dimension of layout")
    return center


def start_positions(nodes: list, pos, fixed):
    """The host side of the spring layout's ``pos`` / ``fixed``: ``(given, has, dom_size, fixed_mask)``.  ``given``: float64 ``[n, 2]`` (array
    or tensor) or ``None``; ``has``: bool ``[n]`` array, ``None`` when every node has a position; ``fixed_mask``: bool ``[n]`` array or ``None``."""
    n = len(nodes)
    index = None
    if fixed is not None or isinstance(pos, dict):
        index = {node: i for i, node in enumerate(nodes)}
    given = has = None
    dom_size = 1.0
    if isinstance(pos, dict):
        coords = [float(c) for xy in pos.values() for c in xy]
        dom_size = max(coords) if coords else 1.0                   # (networkx takes max() of an empty dict's values: an error; 1 here)
        given = np.zeros((n, 2), dtype=np.float64)
        has = np.zeros(n, dtype=bool)
        for node, xy in pos.items():
            i = index.get(node)
            if i is not None:
                xy = np.asarray(xy, dtype=np.float64)
                if xy.shape != (2,):
                    raise ValueError(f"pos[{node!r}] must have 2 coordinates, got shape {xy.shape}")
                given[i] = xy
                has[i] = True
    elif pos is not None:
        given = pos.detach() if isinstance(pos, torch.Tensor) else np.asarray(pos, dtype=np.float64)
        if tuple(given.shape) != (n, 2):
            raise ValueError(f"pos must be a dict keyed by node id or an [n, 2] = [{n}, 2] array in index order, got shape {tuple(given.shape)}")
        dom_size = float(given.max()) if n else 1.0
    if dom_size == 0:
        dom_size = 1.0
    mask = None
    if fixed is not None:
        if pos is None:
            raise ValueError("nodes are fixed without positions given")
        mask = np.zeros(n, dtype=bool)
        for node in fixed:
            i = index.get(node)
            if (node not in pos) if isinstance(pos, dict) else (i is None):
                raise ValueError("nodes are fixed without positions given")
            if i is not None:
                mask[i] = True
    if has is not None and bool(has.all()):
        has = None
    return given, has, dom_size, mask


class Layout(object):
    """The layout engine behind :func:`layout` (reference layout.py:135-269): ``nodes`` (ids in index order), ``edge_index`` ``[2, m]`` or
    ``None``, the layout name, ``weight`` (a tensor with one value per stored edge or ``None``) and the layout's own arguments."""

    def __init__(self, nodes: list, edge_index: Optional[torch.Tensor] = None, layout_type: str = "random", weight: Optional[torch.Tensor] = None,
                 *, return_tensor: bool = False, **kwargs):
        self.nodes = nodes
        self.edge_index = torch.empty((2, 0), dtype=torch.long) if edge_index is None else edge_index
        self.weight = weight
        self.layout_type = layout_type.lower() if isinstance(layout_type, str) else layout_type
        self.return_tensor = return_tensor
        self.kwargs = kwargs

    def generate_layout(self):
        if self.layout_type in NAMES_GRID:
            self.layout = self.grid()
        else:
            self.layout = self.generate_nx_layout()
        return self.layout

    def generate_nx_layout(self):
        """Every layout but the grid.  The reference converts to networkx here; the name is kept, networkx is not called."""
        family = layout_family(self.layout_type)
        if family == "grid":
            return self.grid()
        return getattr(self, "_" + family)(**self.kwargs)

    # -------------------------------------------------------------- results
    def _device(self) -> torch.device:
        return _dispatch.compute_device(self.edge_index)

    def _result(self, pos: torch.Tensor):
        if self.return_tensor:
            return pos
        rows = pos.cpu().numpy()
        return {node: rows[i] for i, node in enumerate(self.nodes)}

    def _small(self, center: np.ndarray):
        """n = 0 and n = 1 as networkx answers them: ``{}`` and ``{id: center}``."""
        if self.return_tensor:
            return torch.as_tensor(center, dtype=torch.float64).reshape(1, 2)[:len(self.nodes)].to(self._device())
        return {node: center for node in self.nodes}

    # -------------------------------------------------------------- layouts
    def grid(self):
        """Nodes on a square grid of side ``floor(sqrt(n))`` and width 1, row by row downwards (reference layout.py:249-269)."""
        if len(self.nodes) == 0:
            return self._small(np.zeros(2))
        return self._result(_dispatch.layout_closed_form(_dispatch.LAYOUT_GRID, len(self.nodes), self._device()))

    def _random(self, center=None, dim=2, seed=None):
        center = _center(center, dim)
        if len(self.nodes) == 0:
            return self._small(center)
        return self._result(_dispatch.layout_random(_seed(seed), len(self.nodes), center, self._device()))

    def _circular(self, scale=1, center=None, dim=2):
        center = _center(center, dim)
        n = len(self.nodes)
        if n < 2:
            return self._small(center)
        pos = _dispatch.layout_closed_form(_dispatch.LAYOUT_CIRCULAR, n, self._device())
        return self._result(_dispatch.layout_rescale(pos, scale, center))

    def _spring(self, k=None, pos=None, fixed=None, iterations=50, threshold=1e-4, scale=1, center=None, dim=2, seed=None):
        global last_iterations, last_err
        center = _center(center, dim)
        n = len(self.nodes)
        given, has, dom_size, mask = start_positions(self.nodes, pos, fixed)
        if n < 2:
            return self._small(center)
        dev = self._device()
        adjacency = _dispatch.layout_adjacency(self.edge_index, self.weight, n)
        if given is None:                                           # networkx's dense routine draws in [0, 1), without the center
            start = _dispatch.layout_start(_seed(seed), n, 1.0, (0.0, 0.0), device=dev)
        else:
            start = _dispatch.layout_start(_seed(seed) if has is not None else 0, n, dom_size, center, torch.as_tensor(given),
                                           None if has is None else torch.as_tensor(has), device=dev)
        if k is None:
            k = dom_size / np.sqrt(n) if fixed is not None else math.sqrt(1.0 / n)
        out, last_iterations, last_err = _dispatch.graph_fr_layout(adjacency, start, float(k), None, None, int(iterations), float(threshold),
                                                                   None if mask is None else torch.as_tensor(mask))
        if fixed is None and scale is not None:
            out = _dispatch.layout_rescale(out, scale, center)
        return self._result(out)
