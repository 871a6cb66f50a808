"""Multi-order De Bruijn graph model, API-compatible with ``pathpyG.core.multi_order_model.MultiOrderModel``
for the construction path and the DBGNN export (reference src/pathpyG/core/multi_order_model.py:61-241, 511-554).

Each layer ``k`` is a :class:`Graph` whose nodes are the distinct length-``k`` node sequences observed in the
input (walks or time-respecting paths) and whose weighted edges count their continuations.  All tensor work
(event-graph lift, line-graph lifts, sequence extension, unique/coalesce) runs in HIP kernels; the
higher-order ``IndexMap`` of every layer is created lazily instead of by a Python loop over nodes.
The likelihood / order-selection methods (:243-509) of a device-resident model run on kernels of their own
(csrc/pp_selection.hip: walk counts without lifts, float64 likelihood terms straight from the layers' CSR); host-resident models and
``NATIVE_SELECTION = False`` keep the chain of torch ops, which reuses the lift kernels for its path counts.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
from scipy.stats import chi2

from .. import _dispatch, _hip
from ..algorithms.lift_order import (
    aggregate_edge_index,
    aggregate_node_attributes,
    lift_order_edge_index,
    lift_order_edge_index_weighted,
)
from ..algorithms.temporal import lift_order_temporal
from ..data import Data, Identity, Lazy
from ..utils.dbgnn import generate_bipartite_edge_index
from .graph import Graph
from .index_map import IndexMap
from .path_data import PathData
from .temporal_graph import TemporalGraph

logger = logging.getLogger("pathpyg_amd")

FUSED_BUILDER = True    # from_temporal_graph(max_order=2) on device-resident streams: the node-by-node order-2 builder (pp_debruijn2_*); False = generic kernels
NATIVE_SELECTION = True    # get_mon_dof / the likelihood terms / estimate_order on device-resident models: pp_walk_counts_i64, pp_mon_*_llh_f64; False = torch ops


class MultiOrderModel:
    """Dictionary of De Bruijn graphs ``layers[k]`` for k = 1..max_order."""

    def __init__(self) -> None:
        self.layers: dict[int, Graph] = {}

    def __str__(self) -> str:
        return f"MultiOrderModel with max. order {max(self.layers) if self.layers else 0}"

    def to(self, device) -> "MultiOrderModel":
        for g in self.layers.values():
            g.to(device)
        return self

    @staticmethod
    def iterate_lift_order(
        edge_index: torch.Tensor,
        node_sequence: torch.Tensor,
        mapping: IndexMap,
        edge_weight: torch.Tensor | None = None,
        aggr: str = "src",
        save: bool = True,
    ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None, Graph | None]:
        """One order lift (reference multi_order_model.py:83-122): line-graph lift of ``edge_index``, lifted
        weights, extended instance sequences and — when ``save`` — the aggregated De Bruijn graph."""
        num_instances = node_sequence.size(0)
        if edge_weight is None:
            ho_index = lift_order_edge_index(edge_index, num_nodes=num_instances)
        else:
            ho_index, edge_weight = lift_order_edge_index_weighted(edge_index, edge_weight=edge_weight, num_nodes=num_instances, aggr=aggr)
        node_sequence = _dispatch.extend_node_sequence(edge_index, node_sequence)
        gk = None
        if save:
            gk = aggregate_edge_index(ho_index, node_sequence, edge_weight)
            gk.mapping = IndexMap.from_node_sequence(mapping, gk.data.node_sequence)
        return ho_index, node_sequence, edge_weight, gk

    @staticmethod
    def from_temporal_graph(
        g: TemporalGraph,
        delta: float | int = 1,
        max_order: int = 1,
        weight: str = "edge_weight",
        cached: bool = True,
        event_graph: Optional[torch.Tensor] = None,
    ) -> "MultiOrderModel":
        """De Bruijn layers of the time-respecting paths of ``g`` with waiting time ``delta``
        (reference multi_order_model.py:124-192).  ``cached=False`` keeps only the top layer;
        ``event_graph`` reuses a precomputed ``lift_order_temporal(g, delta)``.

        Same layers as the reference, computed without ever materialising the per-instance node sequences
        (``[E_k, k+1]`` tensors): see :class:`_LiftChain`.  Merged weights are the reference's left-to-right fp32 sums while they
        stay below 2^24.  Beyond, where that sum stalls (ones stop at 16777216.0), a unit-weight edge weighs float32(its count); a
        weighted sum is the float64 sum rounded once for the LONG runs - more than 512 instances on the generic kernels, a first-order
        node pair of more than 128 events on the level-by-level builder, a first-order run of a node with more than 64 out-events on
        the order-2 builder - and the reference's stalled sum for all others, so routes may differ there.  The order-2 builder's layer 2
        through nodes with more than 64 events per side sums in another association (see ``_hip.debruijn2``).  A stream with 2^31 or
        more instances at some order raises ``HipError``."""
        if max_order == 2 and event_graph is None and FUSED_BUILDER:
            # LIFT_ONLY_ORDER2 (off by default): a stream with a very large hub (BASELINE configs[2]'s generator: a node with 2 * 10^6 in-events) costs
            # the order-2 builder's hub kernels 10-11 ms where the level-by-level builder makes both layers in 5.3-5.7 ms — but it makes no GCN
            # plans, and DBGNN.forward building them from the layers' tensors costs 20 ms more than the order-2 builder's own (39 against 25 ms
            # for model + bundle + one step, tools/probes/hub_k2_routes.py): the default serves the DBGNN workflow, the switch a caller who only lifts
            fused = _multi_order_fused(g, delta, 2, weight, cached) if (LIFT_ONLY_ORDER2 and _has_large_hub(g)) else None
            if fused is None:
                fused = _second_order_fused(g, delta, weight, cached)
            if fused is not None:
                return fused
        if max_order >= 3 and FUSED_BUILDER:
            fused = _multi_order_fused(g, delta, max_order, weight, cached, event_graph)
            if fused is not None:
                return fused
        return MultiOrderModel._from_temporal_graph_generic(g, delta, max_order, weight, cached, event_graph)

    @staticmethod
    def _from_temporal_graph_generic(g: TemporalGraph, delta, max_order: int, weight: str, cached: bool, event_graph) -> "MultiOrderModel":
        """:meth:`from_temporal_graph` on the generic kernels, order by order as the reference goes: event graph (``pp_temporal_*``), line-graph
        lifts (``pp_linegraph_*``), coalesce per layer (``pp_coalesce_*``) — any ``max_order``, ``event_graph=``, host-resident streams, weights of
        any dtype, streams the level-by-level builders hand back."""
        m = MultiOrderModel()
        data = g.data if g.data.is_sorted_by_time() else g.data.sort_by_time()
        edge_index = data.edge_index
        n = int(data.num_nodes)
        dev = edge_index.device
        if weight in data:
            edge_weight = data[weight]
        else:
            edge_weight = _hip.UNIT          # the reference's torch.ones(m) (:150-151) as a marker: unit weights stay unit under the "src" lift,
            #                                  and the weight of a merged edge is the length of its run (pp_coalesce_fill, no gather)
        first_order = torch.arange(n, device=dev).unsqueeze(1)
        chain = _LiftChain.first_order(edge_index, first_order, edge_weight, identity_nodes=True, num_first_order=n,
                                       want_pairs=max_order > 1)
        if cached or max_order == 1:
            m.layers[1] = chain.graph
            m.layers[1].mapping = g.mapping
        if max_order > 1:
            ho_index = lift_order_temporal(g, delta) if event_graph is None else event_graph
            chain = chain.to_second_order(edge_index, ho_index,
                                          edge_weight if isinstance(edge_weight, str) else aggregate_node_attributes(ho_index, edge_weight, "src"),
                                          save=cached or max_order == 2, want_edge_ids=max_order > 2)
            if cached or max_order == 2:
                m.layers[2] = chain.graph
                m.layers[2].mapping = IndexMap.from_node_sequence(g.mapping, chain.graph.data.node_sequence)
            for k in range(3, max_order + 1):
                keep = cached or k == max_order
                chain = chain.lift("src", save=keep, want_edge_ids=k < max_order)
                if keep:
                    m.layers[k] = chain.graph
                    m.layers[k].mapping = IndexMap.from_node_sequence(g.mapping, chain.graph.data.node_sequence)
        return m

    @staticmethod
    def from_path_data(path_data: PathData, max_order: int = 1, mode: str = "propagation", cached: bool = True) -> "MultiOrderModel":
        """De Bruijn layers of observed walks (reference multi_order_model.py:194-241).
        ``mode="propagation"`` carries the walk weight along; ``"diffusion"`` splits it by out-degree.

        Propagation mode with ``max_order >= 2`` on a device-resident walk store builds the layers level by level (:func:`_paths_fused`);
        everything else — diffusion, host-resident walks, another weight dtype, ``max_order == 1``, node ids with gaps, a node sequence
        observed at more than 4096 walk positions that all continue — runs on the generic kernels below.  Same layers either way."""
        if max_order >= 2 and mode == "propagation" and FUSED_BUILDER:
            fused = _paths_fused(path_data, max_order, cached)
            if fused is not None:
                return fused
        m = MultiOrderModel()
        walks = path_data.data
        edge_index = walks.edge_index
        node_sequence = walks.node_sequence
        edge_weight = walks.dag_weight.repeat_interleave(walks.dag_num_edges)
        aggr = "src"
        if mode == "diffusion":
            outdeg = _dispatch_degree(edge_index[0], node_sequence.size(0))
            edge_weight = edge_weight / aggregate_node_attributes(edge_index, outdeg, "src")
            aggr = "mul"
        chain = _LiftChain.first_order(edge_index, node_sequence, edge_weight, identity_nodes=False, num_first_order=None,
                                       want_pairs=max_order > 1)
        m.layers[1] = chain.graph
        m.layers[1].mapping = path_data.mapping
        for k in range(2, max_order + 1):
            keep = cached or k == max_order
            chain = chain.lift(aggr, save=keep, want_edge_ids=k < max_order)
            if keep:
                m.layers[k] = chain.graph
                m.layers[k].mapping = IndexMap.from_node_sequence(m.layers[1].mapping, chain.graph.data.node_sequence)
        return m

    # ------------------------------------------------------------------ model selection
    def get_mon_dof(self, max_order: Optional[int] = None, assumption: str = "paths") -> int:
        """Degrees of freedom of the multi-order model up to ``max_order`` (reference multi_order_model.py:243-309).

        "paths": sum over k of the number of length-k paths of the first-order topology minus, per order, the nodes that start at least
        one length-k path (their transition rows sum to one); "ngrams": all ``n^k (n-1)`` combinations.
        A device-resident layer 1 is counted by ``pp_walk_counts_i64``: one int64 vector pushed ``max_order`` times through its CSR gives
        both numbers exactly, in Python ints — no line-graph lift, so orders whose 2^31 or more paths the lifts cannot hold are answered too;
        ``OverflowError`` once a count leaves int64.  Otherwise (host tensors, ``NATIVE_SELECTION = False``) the paths are counted as the
        reference does, by k-1 line-graph lifts of layer 1, and the row constraint by propagating ``starts_k = A starts_{k-1} > 0``."""
        return self._mon_dof(max_order, assumption, None)

    def _mon_dof(self, max_order: Optional[int], assumption: str, memo: Optional[dict]) -> int:
        if max_order is None:
            max_order = max(self.layers)
        if max_order > max(self.layers):
            logger.error("max_order cannot be larger than maximum order of multi-order network")
            raise ValueError("max_order cannot be larger than maximum order of multi-order network")
        g1 = self.layers[1]
        n = int(g1.data.num_nodes)
        dof = n - 1
        if assumption == "paths":
            counts = self._walk_counts(max_order, memo)
            if counts is not None:
                return dof_from_walk_counts(n, counts[0], counts[1], max_order)
            edge_index = g1.data.edge_index
            for k in range(1, max_order + 1):
                if k > 1:
                    num_nodes = 0 if edge_index.numel() == 0 else _dispatch.minmax(edge_index)[1] + 1
                    edge_index = lift_order_edge_index(edge_index, num_nodes)
                dof += int(edge_index.shape[1])                      # number of paths of length k
            dev = _dispatch.compute_device(g1.data.edge_index)
            ptr = g1.row_ptr.to(dev).to(torch.int32)
            col = g1.col.to(dev).to(torch.int32).contiguous()
            starts = torch.ones((n, 1), device=dev)
            for k in range(1, max_order + 1):
                starts = (_hip.spmm(ptr, col, None, n, starts) > 0).to(torch.float32)    # has a length-k path leaving it
                dof -= int(starts.sum().item())
        elif assumption == "ngrams":
            for order in range(1, max_order + 1):
                dof += (n ** order) * (n - 1)
        else:
            logger.error("Unknown assumption %s. Only 'path' and 'ngram' are accepted.", assumption)
            raise ValueError(f"Unknown assumption {assumption}. Only 'path' and 'ngram' are accepted.")
        return int(dof)

    def _walk_counts(self, max_order: int, memo: Optional[dict]):
        """``(totals, starts)`` of layer 1's topology for the orders 1..``max_order`` (``_hip.walk_counts``), from ``memo`` when it holds enough
        orders; ``None``: layer 1 is not on the device, or the switch is off."""
        if not NATIVE_SELECTION:
            return None
        if max_order <= 0:
            return [], []
        if memo is not None and len(memo.get("counts", ((), ()))[0]) >= max_order:
            return memo["counts"]
        csr = _selection_csr(self.layers[1], need_weight=False)
        if csr is None:
            return None
        row_ptr, col, _ = csr
        counts = _hip.walk_counts(row_ptr, col, int(self.layers[1].data.num_nodes), max_order)
        if memo is not None:
            memo["counts"] = counts
        return counts

    def _zeroth_terms(self, dag_graph: Data, memo: Optional[dict]):
        """``(Z, Z0)`` of the walk store from ``pp_mon_zeroth_llh_f64`` or ``None`` (walks not on the device with their stock dtypes, node ids
        with gaps, the switch off): then the torch ops run."""
        if memo is not None and "zeroth" in memo:
            return memo["zeroth"]
        out = None
        if _native_walks(dag_graph):
            out = _hip.mon_zeroth_llh(dag_graph.node_sequence, dag_graph.dag_num_nodes, dag_graph.dag_weight, int(self.layers[1].data.num_nodes))
        if memo is not None:
            memo["zeroth"] = out
        return out

    def _layer_terms(self, dag_graph: Data, order: int, want_intermediate: bool, memo: Optional[dict]):
        """``(T, I)`` of layer ``order`` from ONE ``pp_mon_layer_llh_f64`` call — the top-order term and, with ``want_intermediate``, the
        contribution of every walk's first order-``order`` transition — or ``None`` when the layer or the walks are not on the device with
        their stock dtypes (or the switch is off).  ``I`` is ``None`` when it was not asked for, and when the NEXT layer's ``inverse_idx`` is
        not on the device: the layer's own term stays native, only the intermediate term takes the torch route."""
        key = ("layer", order)
        if memo is not None and key in memo and (memo[key] is None or memo[key][1] is not None or not want_intermediate
                                                 or ("no inverse", order) in memo):
            return memo[key]
        out = None
        if _native_walks(dag_graph):
            csr = _selection_csr(self.layers[order], need_weight=True)
            sel = freq = None
            if csr is not None and want_intermediate:
                inverse = _selection_inverse(self.layers[order + 1])
                if inverse is None:
                    want_intermediate = False
                    if memo is not None:
                        memo["no inverse", order] = True
                else:
                    # first instance of every walk that still has one at this order (reference :352-361): a walk of L nodes holds L - order of them
                    lengths_ho = dag_graph.dag_num_nodes - order
                    keep = lengths_ho > 0
                    kept = lengths_ho[keep]
                    sel = inverse[torch.cumsum(kept, 0) - kept]
                    freq = dag_graph.dag_weight[keep]
            if csr is not None:
                t, i = _hip.mon_layer_llh(csr[0], csr[2], sel, freq)
                out = (t, i if want_intermediate else None)
        if memo is not None:
            memo[key] = out
        return out

    def get_zeroth_order_log_likelihood(self, dag_graph: Data) -> float:
        """Log-likelihood of the walks' first nodes under the node-frequency model (reference multi_order_model.py:311-336).
        On a device-resident walk store whose node ids are exactly 0..n-1: the float64 sum of the same formula (``pp_mon_zeroth_llh_f64``),
        where the torch ops sum in float32.  The kernel takes the walks' first positions from ``dag_num_nodes``, the torch ops from
        ``edge_index``: the store is assumed to be as ``PathData.append_walks`` leaves it, where the two agree."""
        return self._zeroth_order_llh(dag_graph, None)

    def _zeroth_order_llh(self, dag_graph: Data, memo: Optional[dict]) -> float:
        native = self._zeroth_terms(dag_graph, memo)
        if native is not None:
            return native[0]
        frequencies = dag_graph.dag_weight
        is_start = torch.ones(dag_graph.num_nodes, dtype=torch.bool, device=frequencies.device)
        is_start[dag_graph.edge_index[1]] = False
        start_nodes = dag_graph.node_sequence.squeeze()[is_start]
        _, counts = torch.unique(dag_graph.node_sequence, return_counts=True)
        emission = counts / counts.sum()
        return torch.mul(frequencies, torch.log(emission[start_nodes])).sum().item()

    def get_intermediate_order_log_likelihood(self, dag_graph: Data, order: int) -> float:
        """Contribution of the first order-``order`` transition of every walk (reference multi_order_model.py:338-369).
        On a device-resident model: the float64 sum of the same formula (``pp_mon_layer_llh_f64``, the row of a transition found in the
        layer's CSR), where the torch ops sum in float32."""
        return self._intermediate_order_llh(dag_graph, order, None)

    def _intermediate_order_llh(self, dag_graph: Data, order: int, memo: Optional[dict]) -> float:
        native = self._layer_terms(dag_graph, order, True, memo)
        if native is not None and native[1] is not None:
            return native[1]
        frequencies = dag_graph.dag_weight
        lengths_ho = dag_graph.dag_num_nodes - order                 # walks shrink by `order` nodes in order-k encoding
        keep = lengths_ho > 0
        frequencies = frequencies[keep]
        kept = lengths_ho[keep]
        first_of_walk = torch.cumsum(kept, 0) - kept                 # start position of each surviving walk
        probs = self.layers[order].transition_probabilities()[self.layers[order + 1].data.inverse_idx[first_of_walk]]
        return torch.mul(frequencies, torch.log(probs)).sum().item()

    def get_mon_log_likelihood(self, dag_graph: Data, max_order: int = 1) -> float:
        """Log-likelihood of the walks under the multi-order model with layers 0..``max_order``
        (reference multi_order_model.py:371-409): the zeroth-order term, the intermediate terms of the orders below ``max_order`` and the
        top layer's term, added left to right.  On a device-resident model every term is the float64 sum of its formula (see the term
        methods), where the torch ops sum in float32."""
        return self._mon_llh(dag_graph, max_order, None)

    def _mon_llh(self, dag_graph: Data, max_order: int, memo: Optional[dict]) -> float:
        if max_order > 0:
            zeroth = self._zeroth_order_llh(dag_graph, memo)
            intermediate = [self._intermediate_order_llh(dag_graph, order, memo) for order in range(1, max_order)]
            native = self._layer_terms(dag_graph, max_order, False, memo)
            if native is not None:
                return llh_from_terms(zeroth, intermediate, native[0])
            top = self.layers[max_order]
            probs = top.transition_probabilities(edge_attr="edge_weight")
            return llh_from_terms(zeroth, intermediate, (torch.log(probs) * top.data.edge_weight).sum().item())
        native = self._zeroth_terms(dag_graph, memo)
        if native is not None:
            return native[1]
        frequencies = dag_graph.dag_weight
        counts = torch.bincount(dag_graph.node_sequence.squeeze(), frequencies.repeat_interleave(dag_graph.dag_num_nodes))
        emission = counts / counts.sum()
        return torch.mul(torch.log(emission), counts).sum().item()

    def likelihood_ratio_test(self, dag_graph: Data, max_order_null: int = 0, max_order: int = 1, assumption: str = "paths",
                              significance_threshold: float = 0.01) -> tuple:
        """Likelihood-ratio test of order ``max_order`` against ``max_order_null`` (reference multi_order_model.py:411-459):
        ``(null rejected?, p-value)`` with ``x = -2 (log L0 - log L1)`` chi-square distributed in the dof difference.
        The terms the two likelihoods share and the walk counts of the two dof are computed once."""
        return self._ratio_test(dag_graph, max_order_null, max_order, assumption, significance_threshold, {})

    def _ratio_test(self, dag_graph: Data, max_order_null: int, max_order: int, assumption: str, significance_threshold: float, memo: dict) -> tuple:
        if max_order_null >= max_order:
            logger.error("order of null hypothesis must be smaller than order of alternative hypothesis")
            raise ValueError("order of null hypothesis must be smaller than order of alternative hypothesis")
        if max_order > max(self.layers):
            logger.error("order of hypotheses must be smaller than max. order of MultiOrderModel")
            raise ValueError(f"order of hypotheses ({max_order_null} and {max_order}) must be smaller than max. order of "
                             f"MultiOrderModel {max(self.layers)}")
        x = -2 * (self._mon_llh(dag_graph, max_order_null, memo) - self._mon_llh(dag_graph, max_order, memo))
        dof_diff = self._mon_dof(max_order, assumption, memo) - self._mon_dof(max_order_null, assumption, memo)
        p = 1 - chi2.cdf(x, dof_diff)
        return (p < significance_threshold), p

    def estimate_order(self, dag_data: PathData, max_order: Optional[int] = None, significance_threshold: float = 0.01) -> int:
        """Highest order whose layer significantly improves the likelihood of the walks (reference multi_order_model.py:461-509):
        the last k in 2..``max_order`` whose :meth:`likelihood_ratio_test` against k-1 rejects.  One pass: every likelihood term and the
        walk counts are computed once for all the tests (each layer's top and intermediate term come out of one kernel call)."""
        if max_order is None:
            max_order = max(self.layers)
        if max_order > max(self.layers):
            logger.error("max_order cannot be larger than maximum order of multi-order network")
            raise ValueError("max_order cannot be larger than maximum order of multi-order network")
        if max_order <= 1:
            logger.error("max_order must be larger than one")
            raise ValueError("max_order must be larger than one")
        ours = set(self.layers[1].mapping.node_ids)
        if not set(dag_data.mapping.node_ids).issubset(ours):
            logger.error("Input paths do not have same set of nodes as multi-order network")
            raise ValueError("Input paths do not have same set of nodes as multi-order network")
        memo: dict = {}
        self._walk_counts(max_order, memo)                            # all orders in one call; the tests below read prefixes of it
        for k in range(1, max_order):
            if k in self.layers and k + 1 in self.layers:
                self._layer_terms(dag_data.data, k, True, memo)       # T_k and I_k together; T of the top order comes with its test
        accepted = 1
        for k in range(2, max_order + 1):
            if self._ratio_test(dag_data.data, k - 1, k, "paths", significance_threshold, memo)[0]:
                accepted = k
        return accepted

    def sample_walks(self, order: int, num_walks: int, steps: int, start="weighted", seed: Optional[int] = None) -> PathData:
        """``num_walks`` random walks of at most ``steps`` transitions on layer ``order``, weighted by its ``edge_weight``, as first-order
        sequences in a device-resident :class:`PathData` with layer 1's mapping (:class:`pathpyg_amd.processes.RandomWalk`; walks that
        could not take a step are dropped).  The null model of :meth:`estimate_order`: walks from layer k carry order k."""
        from ..processes import RandomWalk
        if order not in self.layers:
            raise ValueError(f"the model has no layer of order {order}")
        layer = self.layers[order]
        weight = "edge_weight" if "edge_weight" in layer.data else None
        return RandomWalk(layer, weight=weight, first_order_mapping=self.layers[1].mapping).run(num_walks, steps, start, seed).to_path_data()

    def _layer_walk(self, order: int):
        """The :class:`~pathpyg_amd.processes.RandomWalk` of layer ``order``, weighted by its ``edge_weight`` if it has one."""
        from ..processes import RandomWalk
        if order not in self.layers:
            raise ValueError(f"the model has no layer of order {order}")
        layer = self.layers[order]
        weight = "edge_weight" if "edge_weight" in layer.data else None
        mapping = self.layers[1].mapping if 1 in self.layers else None
        return RandomWalk(layer, weight=weight, first_order_mapping=mapping)

    def _first_order_result(self, walk, values: torch.Tensor, return_tensor: bool):
        first = walk.first_order(values)
        if return_tensor:
            return first
        return {walk.mapping.to_id(i): v for i, v in enumerate(first.tolist())}

    def pagerank(self, order: int, alpha: float = 0.85, **kw):
        """PageRank of layer ``order`` (:func:`pathpyg_amd.algorithms.pagerank` with the layer's ``edge_weight``; its keyword
        arguments), projected onto first-order nodes: a layer node's rank goes to its LAST first-order node.  Returns
        ``{first-order id: float}`` in index order or, with ``return_tensor=True``, the float64 tensor on the compute device."""
        from ..algorithms.ranking import pagerank
        return_tensor = bool(kw.pop("return_tensor", False))
        walk = self._layer_walk(order)
        kw.setdefault("weight", walk.weight)
        return self._first_order_result(walk, pagerank(walk.graph, alpha, return_tensor=True, **kw), return_tensor)

    def stationary_distribution(self, order: int, **kw):
        """The stationary visitation probabilities of layer ``order`` (:meth:`pathpyg_amd.processes.RandomWalk.stationary_distribution`
        with the layer's ``edge_weight``; its keyword arguments), projected onto first-order nodes.  Returns ``{first-order id: float}``
        or, with ``return_tensor=True``, the float64 tensor on the compute device."""
        return_tensor = bool(kw.pop("return_tensor", False))
        if kw.get("return_iterations"):
            raise ValueError("return_iterations: ask RandomWalk.stationary_distribution of the layer for the count")
        walk = self._layer_walk(order)
        return self._first_order_result(walk, walk.stationary_distribution(**kw), return_tensor)

    def to_dbgnn_data(self, max_order: int = 2, mapping: str = "last", x: torch.Tensor | None = None,
                      x_h: torch.Tensor | None = None) -> Data:
        """Input bundle of :class:`pathpyg_amd.nn.DBGNN` (reference multi_order_model.py:511-554).

        Like the reference, node features default to one-hot matrices (``torch.eye``).  They are stored as deferred
        :class:`~pathpyg_amd.data.Identity` objects: ``DBGNN.forward`` reads the first layers' ``W^T`` through the CSR instead (dropout of
        the identity included) and never makes them, so the default works at any size; reading ``data.x`` / ``data.x_h`` makes the matrix.
        Pass ``x`` / ``x_h`` (``[N, F]`` / ``[U_k, F]``) for features of your own."""
        if max_order not in self.layers:
            logger.error("Higher-order graph of specified order not found.")
            raise ValueError(f"Higher-order graph of order {max_order} not found.")
        g = self.layers[1]
        g_ho = self.layers[max_order]
        n, n_ho = g.data.num_nodes, g_ho.data.num_nodes
        built = self._fused_plans(max_order, mapping)
        dev = built.fo.fwd_ptr.device if built is not None else g.data.edge_index.device
        if x is None:
            x = g.data.x if g.data.x is not None else Identity(n, dev)
        if x_h is None:
            x_h = Identity(n_ho, dev if built is not None else g_ho.data.edge_index.device)
        if built is not None:
            # The layers came out of the order-2 builder together with the plans DBGNN.forward needs (GCN normalisation of both graphs, the
            # bipartite "last" grouping): the bundle hands the plans over and keeps the reference's tensors as deferred views of the layers —
            # a training step that only runs the model never materialises [2, A2] indices (reference multi_order_model.py:511-554 builds
            # them eagerly; PyG's GCNConv re-normalises on every forward)
            u2, a2 = int(n_ho), int(built.sizes["A2"])
            # (the makers hold the layers' tensors / Lazy objects AS THEY ARE NOW, not the bags: a layer edited after bundling does not leak into a
            #  bundle whose plans were accepted for the tensors of this moment)
            ei1, ei2, w2 = g.data.peek("edge_index"), g_ho.data.peek("edge_index"), g_ho.data.peek("edge_weight")

            def now(v):
                return v.resolve() if isinstance(v, Lazy) else v

            out = Data(
                num_nodes=n,
                num_ho_nodes=n_ho,
                x=x,
                x_h=x_h,
                edge_index=Lazy(lambda: now(ei1), (2, u2)),
                edge_index_higher_order=Lazy(lambda: now(ei2), (2, a2)),
                edge_weights=g.data.edge_weight.float(),
                edge_weights_higher_order=Lazy(lambda: now(w2).float(), (a2,)),
                bipartite_edge_index=Lazy(lambda: generate_bipartite_edge_index(g, g_ho, mapping=mapping, device=dev), (2, u2)),
                y=g.data.y,
            )
            names = ("edge_index", "edge_weights", "edge_index_higher_order", "edge_weights_higher_order", "bipartite_edge_index")
            stamp = {name: out.peek(name) for name in names}
            object.__setattr__(out, "_pp_plans", {"fo": built.fo, "ho": built.ho, "bi": built.bip, "stamp": stamp,
                                                  "versions": {k: v._version for k, v in stamp.items() if isinstance(v, torch.Tensor)}})
            return out
        out = Data(
            num_nodes=n,
            num_ho_nodes=n_ho,
            x=x,
            x_h=x_h,
            edge_index=g.data.edge_index,
            edge_index_higher_order=g_ho.data.edge_index,
            edge_weights=g.data.edge_weight.float(),
            edge_weights_higher_order=g_ho.data.edge_weight.float(),
            bipartite_edge_index=generate_bipartite_edge_index(g, g_ho, mapping=mapping, device=dev),
            y=g.data.y,
        )
        # facts DBGNN.forward would otherwise have to verify on the device (every Graph's edge index is row-sorted)
        object.__setattr__(out, "_pp_hints", {
            # the hints describe exactly these tensor objects at these in-place versions; DBGNN.forward ignores them otherwise
            "stamp": tuple((t, t._version) for t in (out.edge_index, out.edge_weights, out.edge_index_higher_order,
                                                     out.edge_weights_higher_order, out.bipartite_edge_index) if t is not None),
            "rows_sorted": True, "bipartite_sources_sorted": mapping in ("last", "first"),
            # temporal models: the order-2 nodes ARE the first-order graph's edges, in its edge order (_LiftChain.to_second_order) -
            # DBGNN.forward then derives the "last" bipartite plan from the first-order plan's destination grouping, no extra sort
            "bipartite_is_fo_edge_heads": bool(mapping == "last" and max_order == 2 and getattr(g_ho, "_nodes_are_fo_edges", False)
                                               and n_ho == g.data.edge_index.size(1))})
        return out


    def _fused_plans(self, max_order: int, mapping: str):
        """The builder result behind ``layers[1]`` / ``layers[2]`` when both still are what :func:`_second_order_fused` made (same objects,
        edge tensors neither replaced nor edited in place) and the bundle asked for is the one its plans describe; else ``None``."""
        rec = getattr(self, "_pp_fused", None)
        if rec is None or max_order != 2 or mapping != "last":
            return None
        built, layers = rec
        for k, (graph, lazies) in layers.items():
            if self.layers.get(k) is not graph:
                return None
            for name, made in lazies.items():
                cur = graph.data.peek(name)
                if isinstance(made, Lazy):
                    if not (cur is made or (made.value is not None and cur is made.value and cur._version == made.version)):
                        return None
                elif not (cur is made[0] and cur._version == made[1]):
                    return None
        return built


def dof_from_walk_counts(n: int, totals: list, starts: list, max_order: int) -> int:
    """Degrees of freedom of the "paths" assumption (reference multi_order_model.py:283-309) from the walk counts of the first-order topology:
    ``n - 1`` for order 0 plus, per order k <= ``max_order``, the walks of length k (``totals[k - 1]``) minus the nodes that start one
    (``starts[k - 1]``: a row of the order-k transition matrix sums to one).  Python ints: exact at any size."""
    return int(n) - 1 + sum(int(t) for t in totals[:max_order]) - sum(int(s) for s in starts[:max_order])


def llh_from_terms(zeroth: float, intermediate: list, top: float) -> float:
    """Log-likelihood of the model with layers 0..k from its terms (reference multi_order_model.py:385-397): the zeroth-order term of the
    walks' first nodes, the intermediate terms of the orders 1..k-1 and the top layer's term, added left to right."""
    llh = zeroth
    for term in intermediate:
        llh += term
    return llh + top


def _still(current, made: Lazy) -> bool:
    """Whether a bag still holds what a builder put there: the deferred tensor itself, or its value, not edited in place since."""
    return current is made or (made.value is not None and current is made.value and current._version == made.version)


# A layer of a fast builder carries `_pp_csr` = (the builder's MultiOrderLayer, the deferred edge_index and the version of the edge_weight it was
# made with, the deferred inverse_idx, the builder's int32 inverse_idx): a second view of the layer beside Graph._csr, valid only while the bag
# still holds exactly those objects.  It stops being used — the kernels then read Graph.row_ptr / col / edge_weight / inverse_idx — when
# data.edge_index, data.edge_weight or data.inverse_idx is REPLACED (assignment, Graph.to / Data.to, clone), when the read edge_index, edge_weight
# or inverse_idx tensor is EDITED IN PLACE (its _version moves), or when data.num_nodes changes.  Nothing else is looked at.
def _note_csr(graph: Graph, b, weight, inverse32=None) -> None:
    """Remember the builder's CSR arrays of a layer for the order-selection kernels (:func:`_selection_csr`), with what tells whether the
    layer's tensors are still the ones they describe.  ``inverse32``: the builder's int32 ``inverse_idx`` behind the bag's deferred int64 view."""
    if isinstance(weight, torch.Tensor) and weight is b.weight:
        d = graph.data
        graph._pp_csr = (b, d.peek("edge_index"), weight._version, d.peek("inverse_idx"), inverse32)


def _builder_csr(graph: Graph):
    """The :class:`~pathpyg_amd._hip.MultiOrderLayer` a fast builder left behind ``graph`` while ``edge_index`` and ``edge_weight`` still are
    what it made (deferred or read, neither replaced nor edited in place); else ``None``."""
    rec = getattr(graph, "_pp_csr", None)
    if rec is None:
        return None
    b, index, weight_version = rec[:3]
    d = graph.data
    weight = d.peek("edge_weight")
    if not isinstance(index, Lazy) or not _still(d.peek("edge_index"), index) or weight is not b.weight or weight._version != weight_version:
        return None
    return b if int(d.num_nodes) == b.n_nodes else None


def _selection_csr(graph: Graph, need_weight: bool):
    """``(row_ptr, col, weight)`` of a device-resident layer for the order-selection kernels: the builder's int32 arrays when the layer came
    out of a fast builder (its deferred ``edge_index`` stays deferred), else ``Graph.row_ptr`` / ``col`` (int64) and ``edge_weight``.
    ``None``: tensors on the host, or (``need_weight``) weights that are not float32."""
    b = _builder_csr(graph)
    if b is not None and b.row_ptr.is_cuda:
        return b.row_ptr[:b.n_nodes + 1], b.col, b.weight
    ei = _dispatch.plain(graph.data.edge_index)
    if not isinstance(ei, torch.Tensor) or not ei.is_cuda or ei.dtype != torch.int64:
        return None
    weight = graph.data.edge_weight
    if need_weight and not (isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 1
                            and weight.numel() == ei.size(1)):
        return None
    return graph.row_ptr, graph.col, weight


def _selection_inverse(graph: Graph):
    """``inverse_idx`` of a device-resident layer as an int32 / int64 vector — the builder's own int32 one while the bag's deferred view of it
    is untouched — or ``None``."""
    rec = getattr(graph, "_pp_csr", None)
    current = graph.data.peek("inverse_idx")
    if rec is not None and rec[4] is not None and isinstance(rec[3], Lazy) and _still(current, rec[3]):
        return rec[4]
    inverse = graph.data.inverse_idx
    if isinstance(inverse, torch.Tensor) and inverse.is_cuda and inverse.dtype in (torch.int32, torch.int64) and inverse.dim() == 1:
        return inverse
    return None


def _native_walks(dag_graph: Data) -> bool:
    """Whether the order-selection kernels take this walk store: the switch is on and the walks' tensors are on the device with their stock dtypes."""
    if not NATIVE_SELECTION:
        return False
    for name, dtype in (("node_sequence", torch.int64), ("dag_num_nodes", torch.int64), ("dag_weight", torch.float32)):
        t = dag_graph.peek(name) if isinstance(dag_graph, Data) else getattr(dag_graph, name, None)
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            return False
    return True


def _csr_rows(ptr: torch.Tensor, total: int) -> torch.Tensor:
    """Row id of every entry of a CSR with int32 row pointers ``ptr`` (int64 [total])."""
    n = ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=ptr.device), (ptr[1:] - ptr[:-1]).long(), output_size=total)


def _fast_stream(g: TemporalGraph, weight: str):
    """``(ei, time, w, n, m)`` of a stream the fast builders (:func:`_second_order_fused`, :func:`_multi_order_fused`) take: edge index and
    timestamps on the device, the weight attribute absent (``w`` None) or float32 on the device, n > 0 nodes, m > 0 events, sorted by time
    (unsorted: one cheap kernel here instead of a builder's whole count pass); else ``None``."""
    data = g.data
    ei = _dispatch.plain(data.edge_index)
    time = data.time
    if ei is None or time is None or not ei.is_cuda or not time.is_cuda:
        return None
    w = None
    if weight in data:
        w = data[weight]
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or not w.is_cuda:
            return None
    n, m = int(data.num_nodes), int(ei.size(1))
    if n == 0 or m == 0 or not data.is_sorted_by_time():
        return None
    return ei, time, w, n, m


def _csr_layers(g: TemporalGraph, ei: torch.Tensor, csr: list, cached: bool, weight2=None, inverse_high=None, gather_concat=None) -> dict:
    """The layers a fast build keeps (all, or with ``cached=False`` the top one) as :class:`~pathpyg_amd.data.Lazy` views of its source-major
    CSR arrays, ``csr[k - 1]`` = layer k (:class:`~pathpyg_amd._hip.MultiOrderLayer`), identical to what the generic kernels produce, made when
    somebody reads them (reference multi_order_model.py:153-191): ``edge_index`` = (row of every CSR entry, column); ``node_sequence`` of layer 1
    = ``arange(n)``, of layer k the sequence of the entry's row in layer k-1 followed by the entry's last node (De Bruijn property: the nodes of
    layer k ARE the edges of layer k-1; for layer 2 that is layer 1's edge itself); ``inverse_idx`` of layer 1 = ``arange(n)``, of layer 2 the
    merged first-order edge of every event, from layer 3 on ``inverse_high(k)``.  ``weight2(edge_index)``: layer 2's merged weights, for a
    builder that does not keep them in the layer's edge order.  ``gather_concat``: what extends the node sequences (default: the HIP kernel
    behind ``_dispatch.gather_concat``; ``distributed.gather_multi_order`` hands its ``ops``' on)."""
    gather_concat = _dispatch.gather_concat if gather_concat is None else gather_concat
    # (the makers capture CSR arrays, plans and other Lazy objects, never the Data bags that hold them: a bag -> Lazy -> closure -> bag cycle would
    #  keep ~4 GB of plans per model alive until the cyclic collector runs — measured: 14.0 -> 20.8 ms per API step from the 11th step on)
    n, dev = csr[0].n_nodes, ei.device
    layers = {}
    index = seq = None
    for k, b in enumerate(csr, start=1):
        prev_index, prev_seq = index, seq
        index = Lazy(lambda b=b: torch.stack((_csr_rows(b.row_ptr, b.n_edges), b.col.long())), (2, b.n_edges))
        weight = b.weight
        if k == 1:
            seq = Lazy(lambda: torch.arange(n, device=dev).unsqueeze(1), (n, 1))
            inverse = Lazy(lambda: torch.arange(n, device=dev), (n,))
        elif k == 2:
            seq = Lazy(lambda first=prev_index: first.resolve().t().contiguous(), (b.n_nodes, 2))

            def inverse_of(first=prev_index):
                # order-2 node of every event = its merged first-order edge (lift_order.py:133 on the [m, 2] instance rows)
                e1 = first.resolve()
                return torch.searchsorted(e1[0] * n + e1[1], ei[0] * n + ei[1])

            inverse = Lazy(inverse_of, (csr[0].n_instances,))
            if weight2 is not None:
                weight = Lazy(lambda index=index: weight2(index.resolve()), (b.n_edges,))
        else:
            def seq_of(prev_index=prev_index, prev_seq=prev_seq, last=csr[k - 2].last):
                # node u of layer k = edge u of layer k-1: the sequence of that edge's source node, then the edge's last node
                return gather_concat(prev_seq.resolve(), prev_index.resolve()[0].contiguous(), last.long())

            seq = Lazy(seq_of, (b.n_nodes, k))
            inverse = Lazy(lambda k=k: inverse_high(k), (csr[k - 2].n_instances,))
        if cached or k == len(csr):
            d = Data(edge_index=index, num_nodes=b.n_nodes, node_sequence=seq, edge_weight=weight, inverse_idx=inverse)
            layers[k] = Graph._from_parts(d, g.mapping if k == 1 else IndexMap.from_node_sequence(g.mapping, seq))
            _note_csr(layers[k], b, weight)
            if k == 2:
                layers[k]._nodes_are_fo_edges = True
    return layers


def _path_csr_layers(mapping: IndexMap, node_sequence: torch.Tensor, csr: list, inverses: dict, cached: bool, gather_concat=None) -> dict:
    """:func:`_csr_layers` for a model of observed walks (reference multi_order_model.py:211-241): the layers a level-by-level build of a walk
    store keeps — layer 1 always (the reference keeps it whatever ``cached`` says), with ``cached=False`` otherwise only the top one — as
    :class:`~pathpyg_amd.data.Lazy` views of the CSR arrays ``csr[k - 1]`` = layer k.  The walks' node ids are 0 .. n - 1 without gaps (the
    builder's precondition), so layer 1's ``node_sequence`` is ``arange(n)`` and its ``inverse_idx`` the walk store's ``node_sequence[:, 0]``;
    ``inverses[k]``: the int32 ``inverse_idx`` of layer k >= 2 as pp_multiorder_paths_inverse left it, widened to int64 when read.  Mappings:
    ``mapping`` for layer 1, ``IndexMap.from_node_sequence(mapping, node sequence of the layer)`` above.  ``gather_concat`` as in
    :func:`_csr_layers`."""
    gather_concat = _dispatch.gather_concat if gather_concat is None else gather_concat
    n, dev = csr[0].n_nodes, node_sequence.device
    positions = node_sequence.size(0)
    layers = {}
    index = seq = None
    for k, b in enumerate(csr, start=1):
        prev_index, prev_seq = index, seq
        index = Lazy(lambda b=b: torch.stack((_csr_rows(b.row_ptr, b.n_edges), b.col.long())), (2, b.n_edges))
        if k == 1:
            seq = Lazy(lambda: torch.arange(n, device=dev).unsqueeze(1), (n, 1))
            inverse = Lazy(lambda: node_sequence[:, 0].clone(), (positions,))
        else:
            if k == 2:
                seq = Lazy(lambda first=prev_index: first.resolve().t().contiguous(), (b.n_nodes, 2))
            else:
                def seq_of(prev_index=prev_index, prev_seq=prev_seq, last=csr[k - 2].last):
                    # node u of layer k = edge u of layer k-1: the sequence of that edge's source node, then the edge's last node
                    return gather_concat(prev_seq.resolve(), prev_index.resolve()[0].contiguous(), last.long())

                seq = Lazy(seq_of, (b.n_nodes, k))
            inv32 = inverses.get(k)
            inverse = None if inv32 is None else Lazy(lambda inv32=inv32: inv32.long(), (inv32.numel(),))
        if cached or k == 1 or k == len(csr):
            d = Data(edge_index=index, num_nodes=b.n_nodes, node_sequence=seq, edge_weight=b.weight, inverse_idx=inverse)
            layers[k] = Graph._from_parts(d, mapping if k == 1 else IndexMap.from_node_sequence(mapping, seq))
            _note_csr(layers[k], b, b.weight, inv32 if k >= 2 else None)
    return layers


def _paths_fused(path_data: PathData, max_order: int, cached: bool):
    """``from_path_data(paths, max_order >= 2, mode="propagation")`` level by level (``_hip.multi_order_paths`` -> ``pp_multiorder_prepare_paths``,
    ``pp_multiorder_step``, ``pp_multiorder_paths_inverse``): no ``[2, E_k]`` instance graphs, one global sort (level 1), every layer's
    ``inverse_idx`` from its closed form on the walks.  ``None``: the builder does not apply — walk tensors not all on the device with their
    stock dtypes (int64 / float32), no edges — or handed the model back (see ``_hip.multi_order_paths``)."""
    walks = path_data.data
    ei = _dispatch.plain(walks.edge_index)
    seq, lengths, weight = walks.node_sequence, walks.dag_num_nodes, walks.dag_weight
    for t, dtype in ((ei, torch.int64), (seq, torch.int64), (lengths, torch.int64), (walks.dag_num_edges, torch.int64), (weight, torch.float32)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            return None
    if ei.dim() != 2 or ei.size(0) != 2 or ei.size(1) == 0 or seq.dim() != 2 or seq.size(1) != 1:
        return None
    lo, hi = _hip.minmax(seq)
    if lo < 0:
        return None
    built = _hip.multi_order_paths(seq, lengths, weight, ei, hi + 1, max_order, want_inverse=True if cached else "top")
    if built is None:
        return None
    csr, inverses = built
    out = MultiOrderModel()
    out.sizes = {"m": int(ei.size(1)), "N": hi + 1, "layers": [(b.n_nodes, b.n_edges, b.n_instances) for b in csr]}
    out.layers = _path_csr_layers(path_data.mapping, seq, csr, inverses, cached)
    return out


def _second_order_fused(g: TemporalGraph, delta, weight: str, cached: bool):
    """``from_temporal_graph(g, delta, max_order=2)`` on the fused order-2 builder (``_hip.debruijn2`` -> ``pp_debruijn2_count / _fill``): ONE pass
    over the stream yields both layers as CSR plans — no event graph, no ``[E_2, 2]`` instance tensors, one read-back.  The reference's layer
    tensors are deferred views of those plans (:func:`_csr_layers`).
    ``None``: the builder does not apply (see :func:`_fast_stream`) or is not the one to use (a contact-shaped stream, ``_hip.debruijn2_wanted``)."""
    stream = _fast_stream(g, weight)
    if stream is None:
        return None
    ei, time, w, n, m = stream
    if not _hip.debruijn2_wanted(m, n):
        return None
    built = _hip.debruijn2(ei, time, n, delta, w, want_weights=True, unsorted_ok=True)
    if built is None:
        return None
    fo, ho = built.fo, built.ho
    u2, a2 = int(built.sizes["U2"]), int(built.sizes["A2"])
    fwd_weight = built.ho_fwd_weight

    def weights2(e2):
        # the builder keeps the merged weights in destination-major order (contiguous stores); the layer lists its edges source-major
        key_fwd = _csr_rows(ho.fwd_ptr, a2) * u2 + ho.fwd_idx.long()                       # ascending: rows ascending, sources ascending inside a row
        return fwd_weight[torch.searchsorted(key_fwd, e2[1] * u2 + e2[0])]

    csr = [_hip.MultiOrderLayer(n_nodes=n, n_edges=u2, n_instances=m, row_ptr=fo.bwd_ptr, col=fo.bwd_idx, weight=built.fo_weight),
           _hip.MultiOrderLayer(n_nodes=u2, n_edges=a2, n_instances=built.sizes["E2"], row_ptr=ho.bwd_ptr, col=ho.bwd_idx)]
    out = MultiOrderModel()
    out.layers = _csr_layers(g, ei, csr, cached, weight2=weights2)
    if cached:
        d1, d2 = out.layers[1].data, out.layers[2].data
        out._pp_fused = (built, {1: (out.layers[1], {"edge_index": d1.peek("edge_index"), "edge_weight": (built.fo_weight, built.fo_weight._version)}),
                                 2: (out.layers[2], {"edge_index": d2.peek("edge_index"), "edge_weight": d2.peek("edge_weight")})})
    out.sizes = dict(built.sizes)
    return out


LARGE_HUB_EVENTS = 65536
LIFT_ONLY_ORDER2 = False     # from_temporal_graph(max_order=2) on a stream with a node of LARGE_HUB_EVENTS events: True = the level-by-level builder (no GCN plans)
_INT32_ROWS = _hip._INT32_ROWS    # instances one step of the level-by-level builder numbers, and rows the generic kernels' int32 arrays hold
PASS_INSTANCES = _INT32_ROWS      # from_temporal_graph(max_order >= 3): a level with more instances than this (and any level one step cannot number) is built in passes over ranges of its types (core/multi_order_passes.py); smaller = less memory per step


def _has_large_hub(g: TemporalGraph) -> bool:
    """Whether some node of a device-resident stream has ``LARGE_HUB_EVENTS`` or more in- or out-events (two histograms and one read-back, kept
    on the graph object for the tensors they were taken from)."""
    ei = _dispatch.plain(g.data.edge_index)
    if ei is None or not ei.is_cuda or ei.numel() == 0 or ei.size(1) < LARGE_HUB_EVENTS:
        return False
    key = (id(ei), ei._version, int(g.data.num_nodes))
    kept = getattr(g, "_pp_max_degree", None)
    if kept is None or kept[0] != key:
        n = int(g.data.num_nodes)
        ei = ei.contiguous()
        most = int(torch.maximum(_hip.degree(ei[0], n).max(), _hip.degree(ei[1], n).max()))
        kept = g._pp_max_degree = (key, most)
    return kept[1] >= LARGE_HUB_EVENTS


def _multi_order_fused(g: TemporalGraph, delta, max_order: int, weight: str, cached: bool, event_graph=None):
    """``from_temporal_graph(g, delta, max_order >= 3)`` level by level (``_hip.multi_order_temporal`` -> ``pp_multiorder_prepare`` / ``_step``): every
    layer comes out as source-major CSR with merged weights, the reference's layer tensors are deferred views of it (:func:`_csr_layers`), the
    ``inverse_idx`` of the layers from 3 on comes from the generic kernels (:func:`_generic_inverses`).
    ``event_graph``: a given ``lift_order_temporal(g, delta)`` — its edges are the continuation windows (``pp_multiorder_prepare_graph``).
    A level with more than ``PASS_INSTANCES`` instances (default: 2^31 - 16; one step numbers one less) is built in passes over ranges of its types
    (``core/multi_order_passes.py``); ``sizes["passes"]`` holds the number of parts per layer — all ones when no level reached the budget —
    and ``sizes["layers"]`` the true instance counts as Python ints.
    ``None``: the builder does not apply (see :func:`_fast_stream`; a layer without edges, a node sequence with more than 4096 continuations,
    a layer with 2^31 - 16 or more edges, an event graph that is not sorted by source)."""
    stream = _fast_stream(g, weight)
    if stream is None:
        return None
    ei, time, w, n, m = stream
    if event_graph is not None:
        event_graph = _dispatch.plain(event_graph)
        if not isinstance(event_graph, torch.Tensor) or not event_graph.is_cuda or event_graph.dim() != 2 or event_graph.size(0) != 2:
            return None
    passes: list = []
    built = _hip.multi_order_temporal(ei, time, n, delta, w, max_order, event_graph=event_graph, pass_instances=PASS_INSTANCES, passes=passes,
                                       unsorted_ok=True)
    if built is None:
        return None
    out = MultiOrderModel()
    out.sizes = {"m": m, "N": n, "layers": [(b.n_nodes, b.n_edges, b.n_instances) for b in built], "passes": passes}
    out.layers = _csr_layers(g, ei, built, cached, inverse_high=_generic_inverses(g, delta, max_order, weight, cached, event_graph,
                                                                                  instances=[b.n_instances for b in built]))
    return out


def _generic_inverses(g: TemporalGraph, delta, max_order: int, weight: str, cached: bool, event_graph, instances=None):
    """``k -> inverse_idx`` of the layers from 3 on of a level-by-level model.  It numbers the reference's order-k INSTANCES (edges of the
    order-(k-1) instance graph, lexicographic), which only the generic kernels make: ONE generic build of the same layers, on first use,
    serves every layer of the model (one per layer would run K - 2 of them); only its inverse maps are kept.
    ``instances``: the instance counts of the layers 1.. (``sizes["layers"]``'s third entries).  The generic kernels hold fewer than
    ``_INT32_ROWS`` instances per order, a model built in passes may have more: the shared build stops at the highest order below the
    limit, and reading ``inverse_idx`` of a layer at or beyond the first order that reaches it raises ``RuntimeError`` instead of starting
    a build that cannot succeed.  Nothing is decided before the first read: ``Graph.to``, ``MultiOrderModel.to`` and pickling keep the value
    deferred."""
    kept = {}

    def inverse_of(k):
        reach = max_order
        for j, count in enumerate(instances or (), start=1):
            if count >= _INT32_ROWS:
                reach = min(reach, j - 1)
                break
        if k > reach:
            raise RuntimeError(f"inverse_idx of layer {k}: layer {reach + 1} has {instances[reach]} instances, and the generic kernels that number "
                               f"a layer's instances hold fewer than {_INT32_ROWS} (2^31 - 16) of them")
        if not kept:
            model = MultiOrderModel._from_temporal_graph_generic(g, delta, reach, weight, cached, event_graph)
            kept.update((j, layer.data.inverse_idx) for j, layer in model.layers.items() if j >= 3)
        return kept[k]

    return inverse_of


class _LiftChain:
    """State of the order-k instance graph while climbing orders, WITHOUT per-instance node sequences.

    The reference extends an ``[instances, k]`` node-sequence tensor at every order and runs ``torch.unique(dim=0)``
    on it (multi_order_model.py:114, lift_order.py:133).  The same node numbering follows from two vectors per
    order: ``inv[i]`` = De Bruijn node of instance i (its lexicographic rank) and ``last[i]`` = its last first-order
    node.  An order-(k+1) instance is an edge (a -> b) of the order-k instance graph; its node sequence is
    ``seq(a) ++ last[b]``, so its lexicographic rank is the rank of the PAIR ``(inv[a], last[b])`` — a 2-column unique
    instead of a (k+1)-column one — and the distinct sequences are ``unique_k[first] ++ second`` for the distinct pairs.
    When layer k has been aggregated even that sort is unnecessary: the pair ``(inv[a], last[b])`` determines and is determined by
    the layer-k edge ``(inv[a], inv[b])``, so the order-(k+1) nodes are layer k's merged edges in coalesce order and the inverse map
    of that coalesce (``edge_ids``) is the next ``inv``; the 2-column unique remains for ``cached=False`` (layer k not built).
    """

    def __init__(self, index, inv, last, unique_nodes, weight, graph, edge_ids=None):
        self.index = index              # [2, E_k] edges between order-k instances (source-sorted)
        self.inv = inv                  # [M_k] instance -> De Bruijn node id
        self.last = last                # [M_k] last first-order node of every instance
        self.unique_nodes = unique_nodes  # [U_k, k]
        self.weight = weight            # [E_k] or None
        self.graph = graph              # aggregated layer k (or None when not saved)
        # [E_k] position of every instance edge's merged edge in layer k (the inverse map of its coalesce) or None.  De Bruijn property:
        # the order-(k+1) nodes ARE the merged edges of layer k, in the same lexicographic order - so this is the next order's `inv`,
        # and the next order needs no unique over its node sequences at all (reference: torch.unique(dim=0), lift_order.py:133)
        self.edge_ids = edge_ids

    @staticmethod
    def first_order(edge_index, node_sequence, edge_weight, identity_nodes: bool, num_first_order, want_pairs: bool):
        from ..algorithms.lift_order import _aggregate_with_known_nodes
        if identity_nodes:       # temporal graphs: node_sequence = arange(N): every node distinct, already ordered
            unique_nodes = node_sequence
            inv = torch.arange(num_first_order, device=edge_index.device)
        else:
            unique_nodes, inv = _dispatch.unique_rows(node_sequence)
        out = _aggregate_with_known_nodes(edge_index, 1, node_sequence, unique_nodes, inv, edge_weight, "sum", want_inverse=want_pairs)
        graph, edge_ids = out if want_pairs else (out, None)
        if not identity_nodes and edge_ids is not None:
            # Layer 1 of a path model uses the walk node ids AS GIVEN (reference quirk, lift_order.py:135-136), while `unique_nodes` is
            # indexed by RANK.  The shortcut of lift() (order-(k+1) nodes = layer k's merged edges) looks layer-1 edges up in
            # `unique_nodes`, which is only right when id == rank, i.e. the ids are exactly 0..U-1; otherwise the next lift takes the
            # 2-column unique over (rank of prefix, last node), which is id-agnostic.
            u = unique_nodes.size(0)
            ids = _dispatch.plain(unique_nodes).reshape(-1)
            if u and not bool((ids == torch.arange(u, device=ids.device)).all()):
                edge_ids = None
        return _LiftChain(edge_index, inv, _dispatch.plain(node_sequence).reshape(-1), unique_nodes, edge_weight, graph, edge_ids)

    def to_second_order(self, event_index, ho_index, ho_weight, save: bool, want_edge_ids: bool = False):
        """Temporal special case: the order-2 instances are the events themselves, their distinct (src, dst) pairs are
        layer 1's merged edges (already sorted), and ``edge_ids`` from layer 1's coalesce is their inverse map."""
        from ..algorithms.lift_order import _aggregate_with_known_nodes
        unique_nodes = self.graph.data.edge_index.t().contiguous()
        inv = self.edge_ids
        # a successor of node (a, b) is a node (b, c): all of them sit in the contiguous id block of the pairs that start with b
        merged = _dispatch.plain(self.graph.data.edge_index)
        blocks = _dispatch.successor_blocks(merged[0], self.unique_nodes.size(0), merged[1]) if save and merged.size(1) else None
        graph = edge_ids = None
        if save:
            out = _aggregate_with_known_nodes(ho_index, 2, None, unique_nodes, inv, ho_weight, "sum", col_block=blocks, want_inverse=want_edge_ids)
            graph, edge_ids = out if want_edge_ids else (out, None)
            graph._nodes_are_fo_edges = True          # node u of this layer = edge u of layer 1 (same lexicographic order)
        return _LiftChain(ho_index, inv, _dispatch.plain(event_index)[1], unique_nodes, ho_weight, graph, edge_ids)

    def lift(self, aggr: str, save: bool, want_edge_ids: bool = False):
        from ..algorithms.lift_order import _aggregate_with_known_nodes
        num_instances = self.inv.numel()
        if self.weight is None or (isinstance(self.weight, str) and aggr in ("src", "dst", "max", "mul")):      # (unit weights stay unit)
            ho_index, weight = lift_order_edge_index(self.index, num_nodes=num_instances), self.weight
        else:
            w_inst = self.weight
            if isinstance(w_inst, str):            # the UNIT marker under an aggregation that does not preserve it ("add": 1 + 1 = 2): the ones vector
                w_inst = torch.ones(num_instances, dtype=torch.float32, device=_dispatch.plain(self.index).device)      # the reference starts from
            ho_index, weight = lift_order_edge_index_weighted(self.index, w_inst, num_nodes=num_instances, aggr=aggr)
        last = aggregate_node_attributes(self.index, self.last, "dst")                 # last node of every new instance
        k = self.unique_nodes.size(1)
        if self.graph is not None and self.edge_ids is not None:
            # the new nodes ARE layer k's merged edges (same lexicographic order): sequence = prefix node's sequence ++ last node of the
            # suffix node; the coalesce inverse of layer k numbers the new instances - no sort of the instances' node sequences
            merged = _dispatch.plain(self.graph.data.edge_index)
            inv = self.edge_ids
            prefix, suffix = merged[0].contiguous(), merged[1].contiguous()
            tail = _dispatch.plain(self.unique_nodes)[:, -1].contiguous()
            unique_nodes = _dispatch.gather_concat(self.unique_nodes, prefix, aggregate_node_attributes(merged, tail, "dst"))
        else:
            pairs = _dispatch.gather_concat(self.inv.unsqueeze(1), _dispatch.plain(self.index)[0], last)     # (inv[a], last[b])
            hi = max(self.unique_nodes.size(0), int(_dispatch.minmax(self.unique_nodes)[1]) + 1 if self.unique_nodes.numel() else 1)
            unique_pairs, inv = _dispatch.unique_rows(pairs, (0, max(hi - 1, 0)))
            unique_nodes = _dispatch.gather_concat(self.unique_nodes, unique_pairs[:, 0], unique_pairs[:, 1])
            prefix = unique_pairs[:, 0].contiguous()
            suffix = None
            if save and inv.numel():
                # every successor of a new node P starts with P's order-k SUFFIX node, i.e. the order-k node of the second instance of
                # any edge a -> b that realises P
                suffix = torch.empty(unique_pairs.size(0), dtype=torch.int64, device=inv.device)
                suffix[inv] = self.inv[_dispatch.plain(self.index)[1]]
        graph = edge_ids = None
        if save:
            # the new nodes are numbered by (order-k prefix node, last node): all successors of P sit in the id block of P's suffix node
            blocks = _dispatch.successor_blocks(prefix, self.unique_nodes.size(0), suffix) if inv.numel() else None
            out = _aggregate_with_known_nodes(ho_index, k + 1, None, unique_nodes, inv, weight, "sum", col_block=blocks, want_inverse=want_edge_ids)
            graph, edge_ids = out if want_edge_ids else (out, None)
        return _LiftChain(ho_index, inv, last, unique_nodes, weight, graph, edge_ids)


def _dispatch_degree(index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """Out-degree histogram as a float tensor on the input's device (PyG ``degree``, multi_order_model.py:220)."""
    dev = _dispatch.compute_device(index)
    deg = _hip.degree(_dispatch.plain(index).to(dev).contiguous(), num_nodes)
    return deg.to(torch.float32).to(index.device)
