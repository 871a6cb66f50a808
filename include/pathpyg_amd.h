/* pathpyg_amd — C ABI of the MI355X-native (gfx950) higher-order graph engine.
 *
 * This is the drop-in boundary for ONE hot path of pathpy/pathpyG: the k-th order De Bruijn lift
 * of temporal edge streams / walk data and the DBGNN forward/backward that consumes it.  The
 * reference has no FFI seam of its own (it is pure Python on torch + torch_geometric), so every
 * entry point below names the reference function (file:line, relative to the pathpyG repository
 * root) whose tensor work it replaces; the Python shims in pathpyg_amd/ keep the reference's
 * signatures and call these through ctypes.
 *
 * Conventions
 *   - plain C, no torch types: raw DEVICE pointers, element counts, a hipStream_t passed as void*.
 *   - every function returns PP_OK (0) or a negative PP_ERR_* code; pp_last_error() gives the text.
 *   - index tensors at the boundary are int64 row-major [2,E] exactly like the reference;
 *     internal ids are 32-bit, so element counts per call must stay below 2^31 (PP_ERR_TOO_LARGE).
 *   - all memory is owned by the caller (PyTorch's caching allocator in the Python shims).
 *     Scratch comes from a caller-provided workspace sized by the matching *_ws_bytes() query.
 *   - data-dependent output sizes use two calls: *_count leaves its state in the workspace and
 *     writes the size to a device scalar; the caller reads it (one 8-byte D2H copy), allocates the
 *     output and calls *_fill with the SAME workspace.
 *   - everything is asynchronous on `stream`; nothing here synchronises the device.
 */
#ifndef PATHPYG_AMD_H
#define PATHPYG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_VERSION 100 /* 0.1.0 */

typedef void* pp_stream_t; /* hipStream_t */

enum pp_status { PP_OK = 0, PP_ERR_HIP = -1, PP_ERR_ARG = -2, PP_ERR_WORKSPACE = -3, PP_ERR_TOO_LARGE = -4 };

/* element types of caller tensors */
enum pp_dtype { PP_I32 = 0, PP_I64 = 1, PP_F32 = 2, PP_F64 = 3 };

/* per-edge attribute from the two endpoints: reference aggregate_node_attributes,
 * src/pathpyG/algorithms/lift_order.py:33-44 */
enum pp_edge_aggr { PP_AGGR_SRC = 0, PP_AGGR_DST = 1, PP_AGGR_MAX = 2, PP_AGGR_MUL = 3, PP_AGGR_ADD = 4 };

/* duplicate-edge reduction: reference aggregate_edge_index(aggr=...), lift_order.py:139-144 (PyG coalesce) */
enum pp_reduce { PP_REDUCE_SUM = 0, PP_REDUCE_MEAN = 1, PP_REDUCE_MIN = 2, PP_REDUCE_MAX = 3 };

/* how `delta` reached torch.tensor(delta) in the reference (src/pathpyG/algorithms/temporal.py:30,43):
 * the threshold t+delta and the <= comparison are evaluated in torch's promoted dtype. */
enum pp_delta_kind { PP_DELTA_I64 = 0, PP_DELTA_F32 = 1, PP_DELTA_F64 = 2 };

int pp_version(void);
const char* pp_last_error(void);
/* Concurrency between two HIP streams of one process (no reference counterpart: the reference runs nn/dbgnn.py:130-145 — the first-order
 * stack, then the higher-order stack — as one serial chain of torch ops).  The fused layer kernels launch PERSISTENT grids sized to the
 * workgroups that are resident at once, which leaves no slot for a kernel of another stream.  pp_set_launch_share(s) lets the persistent
 * launches of the CALLING THREAD take only s per mille of those slots (1..1000, default 1000) and returns the previous value. */
int pp_set_launch_share(int per_mille);
/* workgroups of the calling thread's most recent persistent launch (0 before the first one) */
int64_t pp_last_persistent_grid(void);

/* ------------------------------------------------------------------ primitives (pp_scan.hip, pp_sort.hip) */

/* torch_geometric.utils.cumsum as used at lift_order.py:74,77: out[0..n] = exclusive prefix sums, out[n] = total */
size_t pp_scan_ws_bytes(int64_t n);
int pp_exclusive_scan_i32(const int32_t* in, int64_t n, int64_t* out, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_exclusive_scan_i64(const int64_t* in, int64_t n, int64_t* out, void* ws, size_t ws_bytes, pp_stream_t stream);

/* torch_geometric.utils.degree(index, num_nodes) as used at lift_order.py:65: bins[v] = #occurrences of v */
int pp_degree_i64(const int64_t* index, int64_t n, int64_t num_bins, int32_t* bins, pp_stream_t stream);

/* out2 = {min, max} of a (INT64_MAX, INT64_MIN when n == 0) */
int pp_minmax_i64(const int64_t* a, int64_t n, int64_t* out2, pp_stream_t stream);

/* stable LSD radix sort of (key, 32-bit value) pairs on key bits [begin_bit, end_bit);
 * vals_in == NULL means values 0..n-1 (argsort).  Replaces torch.argsort / index_sort / torch.unique's sort
 * (temporal_graph.py:58, lift_order.py:133,139, graph.py:103,115).  in/out buffers must differ. */
size_t pp_sort_ws_bytes(int64_t n, int key_bytes);
int pp_sort_pairs_u32(const uint32_t* keys_in, const uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, int64_t n,
                      int begin_bit, int end_bit, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_sort_pairs_u64(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out, int64_t n,
                      int begin_bit, int end_bit, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ fused order-2 De Bruijn builder (pp_debruijn.hip) */

/* MultiOrderModel.from_temporal_graph(g, delta, max_order=2) (src/pathpyG/core/multi_order_model.py:124-192: lift_order_temporal,
 * algorithms/temporal.py:17-54, + aggregate_edge_index for layers 1 and 2, algorithms/lift_order.py:109-152) together with what
 * DBGNN.forward derives from the two layers on every call (gcn_norm through GCNConv, src/pathpyG/nn/dbgnn.py:104-114,130-140) and the
 * bipartite "last" index (utils/dbgnn.py:10-46) — node by node, without materialising the event graph, in three calls:
 *   pp_debruijn2_lists  the two sorts of the events (out-lists, in-lists), hub classification -> 16 int64 statistics copied to `host_stats`
 *                       (pinned host memory; the copy is asynchronous and followed by the out-side kernel of the ordinary nodes, so that
 *                       pp_debruijn2_wait — the ONE call of this library that blocks — returns while the GPU is still busy);
 *   pp_debruijn2_count  everything up to the sizes (the first five int64 of ws).  `host_result` (pinned int64 [154], may be NULL): the whole result
 *                       header is copied there asynchronously, the first size-independent kernel of the fill pass is queued behind the copy,
 *                       pp_debruijn2_wait returns when the copy has landed (NULL: the caller reads the header from ws itself);
 *   pp_debruijn2_fill   both plans (`rows_packed` = 1 when the count call was given a host_result).
 * Same inputs as pp_temporal_count (time-sorted events, delta as torch.tensor(delta) sees it); weight: NULL (every event weighs 1: the
 * reference's default torch.ones) or float32 [m].  Results are identical, array by array, to pp_coalesce_* (layer 1) -> pp_temporal_* ->
 * pp_coalesce_* (layer 2) -> pp_gcn_plan x 2 on the same stream (bit for bit where the partial sums are exact: see "hub nodes" in
 * pp_debruijn.hip for streams with non-integer weights on nodes of more than 64 events).
 * HUB NODES: a node with more than 64 in- or more than 64 out-events is worked on by several waves (chunks of 256 in-events) instead of
 * one; host_stats = {hub nodes, (out-hubs << 32) | their out-events, tasks, part columns, -, longest rows (4), longest in-list, longest
 * out-list, ...} sizes the extra workspace: pp_debruijn2_hub_ws_bytes(out-hub events, out-hubs, part columns); the same five numbers go to
 * count and fill (all 0 and hub_ws NULL when there is no hub).  After count the hub block (ws int64 [138 .. 154)) also holds [4] the lifted
 * pairs through hub nodes (E2 = ws[3] + that) and [5..8] the longest order-2 destination- / source-major and first-order destination- /
 * source-major row among the hubs' rows (the caller's chunked pre-pass for rows beyond 512 entries, pp_spmm_heavy_f32).
 * Order-2 node u = first-order edge u (lexicographic (src, dst) order).  Outputs, all int32 / float32:
 *   count phase (capacities in brackets; U2 = order-2 nodes, A2 = order-2 edges, A1 = U2 = first-order edges):
 *     fo_bwd_ptr [N+1], fo_bwd_idx [m], fo_w [m]     source-major first-order graph: successors of every node + merged weights (first U2 entries)
 *     fo_fwd_ptr [N+1]                                destination-major row pointers of the first-order graph
 *     ho_fwd_ptr [m+1], ho_bwd_ptr [m+1]              row pointers of the order-2 graph, destination- / source-major (first U2+1 entries; constant after)
 *     ho_deg [m], fo_deg [N]                          weighted in-degree incl. the self loop of gcn_norm (add_remaining_self_loops, fill 1)
 *   the first five int64 of ws = {U2, status, A2, E2 (without the hubs' pairs), A1}; status bit 0: node index outside [0, N); bit 1: time
 *     not ascending; bit 2: (partition shards only) a node has more than 64 in- or out-events.
 *   fill phase: ho_fwd_idx/val [A2] (in-edges of every order-2 node, ascending source), ho_bwd_idx/val [A2], ho_self [U2];
 *     fo_fwd_idx/val [A1], fo_dst_order [A1] (edge id = order-2 node id of every in-edge: the bipartite "last" grouping),
 *     fo_bwd_val [U2], fo_self [N].  Values are the normalised coefficients d_src^-1/2 w d_dst^-1/2 (0 on self-loop entries).
 *     num_ho_edges = A2; pair_scratch: 8 * A2 bytes of device scratch (the source-major rows are scattered as 8-byte pairs, then split).
 *     ho_fwd_w [A2] (optional, may be NULL): the merged weights THEMSELVES (lift_order.py:139, coalesce "sum") in destination-major order —
 *     what MultiOrderModel.layers[2].data.edge_weight is derived from when a caller reads it. */
size_t pp_debruijn2_ws_bytes(int64_t m, int64_t num_nodes);
size_t pp_debruijn2_hub_ws_bytes(int64_t hub_out_events, int64_t out_hubs, int64_t hub_parts);
int pp_debruijn2_lists(const int64_t* edge_index, const void* time, int time_dtype, int64_t m, int64_t num_nodes, const float* weight, void* ws,
                       size_t ws_bytes, int64_t* host_stats, pp_stream_t stream);
int pp_debruijn2_wait(void);
int pp_debruijn2_count(int time_dtype, int64_t m, int64_t num_nodes, int delta_kind, int64_t delta_i, double delta_f, const float* weight,
                       int32_t* fo_bwd_ptr, int32_t* fo_bwd_idx, float* fo_w, int32_t* fo_fwd_ptr, int32_t* ho_fwd_ptr, int32_t* ho_bwd_ptr,
                       float* ho_deg, float* fo_deg, void* ws, size_t ws_bytes, int64_t hub_nodes, int64_t out_hubs, int64_t hub_out_events,
                       int64_t hub_tasks, int64_t hub_parts, void* hub_ws, size_t hub_ws_bytes, int64_t* host_result, pp_stream_t stream);
int pp_debruijn2_fill(int time_dtype, int64_t m, int64_t num_nodes, int delta_kind, int64_t delta_i, double delta_f, const float* weight,
                      const int32_t* fo_bwd_ptr, const int32_t* fo_bwd_idx, const float* fo_w, const int32_t* fo_fwd_ptr, const int32_t* ho_fwd_ptr,
                      const int32_t* ho_bwd_ptr, const float* ho_deg, const float* fo_deg, int64_t num_ho_edges, int32_t* ho_fwd_idx, float* ho_fwd_val,
                      int32_t* ho_bwd_idx, float* ho_bwd_val, float* ho_self, int32_t* fo_fwd_idx, float* fo_fwd_val, int32_t* fo_dst_order,
                      float* fo_bwd_val, float* fo_self, float* ho_fwd_w, void* pair_scratch, void* ws, size_t ws_bytes, int64_t hub_nodes,
                      int64_t out_hubs, int64_t hub_out_events, int64_t hub_tasks, int64_t hub_parts, void* hub_ws, size_t hub_ws_bytes,
                      int rows_packed, pp_stream_t stream);
/* pp_debruijn2_wait + pp_debruijn2_fill in ONE call, for a caller that allocated the A2-sized outputs ahead of the size read-back with a guessed
 * capacity (ho_edge_capacity entries; pair_scratch 8 * capacity bytes): waits for the header pp_debruijn2_count copied to host_result, and launches
 * the fill at once when the stream is good (status 0) and A2 fits — *launched = 1 — so that nothing of the caller's host code sits between the
 * read-back and the fill; otherwise *launched = 0 and nothing was queued (the caller reads the header, allocates exactly and calls
 * pp_debruijn2_fill, or reports the status). */
int pp_debruijn2_fill_ready(int time_dtype, int64_t m, int64_t num_nodes, int delta_kind, int64_t delta_i, double delta_f, const float* weight,
                            const int32_t* fo_bwd_ptr, const int32_t* fo_bwd_idx, const float* fo_w, const int32_t* fo_fwd_ptr, const int32_t* ho_fwd_ptr,
                            const int32_t* ho_bwd_ptr, const float* ho_deg, const float* fo_deg, int64_t ho_edge_capacity, int32_t* ho_fwd_idx,
                            float* ho_fwd_val, int32_t* ho_bwd_idx, float* ho_bwd_val, float* ho_self, int32_t* fo_fwd_idx, float* fo_fwd_val,
                            int32_t* fo_dst_order, float* fo_bwd_val, float* fo_self, float* ho_fwd_w, void* pair_scratch, void* ws, size_t ws_bytes,
                            int64_t hub_nodes, int64_t out_hubs, int64_t hub_out_events, int64_t hub_tasks, int64_t hub_parts, void* hub_ws,
                            size_t hub_ws_bytes, int rows_packed, const int64_t* host_result, int64_t* launched, pp_stream_t stream);

/* The same builder on ONE RANK of a node-range partition (the lift shards by edge range, the DBGNN by destination-node
 * partition; no reference counterpart — the reference is single-process).  Rank `rank` owns the first-order nodes
 * [node_lo, node_lo + n_own) = cuts[rank] .. cuts[rank + 1] (cuts: device int64 [world + 1]) and is handed the time-sorted events that start
 * or end in that range (node ids stay global).  Every order-2 edge (a,b) -> (b,c) is born on the owner of its MIDDLE node b, which owns the
 * rows (b, .): no lifted pair and no order-2 node id ever crosses a link.  Sources (a, b) with a foreign a are halo rows, numbered behind
 * the U2 owned rows in (owner of a, b, a) order.  The owned rows are numbered in SEND ORDER: the rows (b, c) other ranks gather from come
 * first, grouped by the owner of c and ordered by (c, b) — the receiver's halo order —, so the send list of every layer exchange is the
 * contiguous prefix [0, rows sent) of a row matrix (no pack, no ids, no request round: one all-to-all of rows fills the peers' halos); rows
 * nobody gathers from follow.  fo_bwd_idx / fo_w are in that local order (fo_bwd_ptr stays lexicographic: block sizes per node);
 * send_slot [m]: local row -> its position in the prefix, -1 behind it; row_of [m]: local row -> lexicographic row (global id - first owned id).
 * In that order ALL rows are grouped by their successor c, so the bipartite "last" plan (utils/dbgnn.py:10-46) of the shard needs no sort either:
 * destinations = all first-order nodes in the rank-major padded layout (node c of rank r at r * pad_rows + c - cuts[r]; pad_rows >= the largest
 * range), bip_fwd_ptr [world * pad_rows + 1] / bip_fwd_idx [m] (local rows per destination), bip_bwd_ptr [m + 1] / bip_bwd_idx [m] (one
 * destination per row), bip_self [world * pad_rows] (in-degrees) — all written by the count phase.  The first 8 int64 of ws = {U2, status, A2, E2, A1, halo rows, rows sent, -}, then recv_ptr [world + 1] and
 * send_ptr [world + 1] (rows from / to every rank, as offsets).  Between count and fill the caller fetches ho_deg of its halo rows
 * (ho_deg[U2 ..]) from their owners and all-gathers fo_deg (the count pass fills the owned entries of the [num_nodes] array).  Fill: the
 * order-2 plan over the local source space [owned | halo] as in pp_debruijn2_fill, and the rank's FIRST-ORDER SHARD with a dense halo — local
 * source space [owned | ids below node_lo | ids from node_lo + n_own on] (num_nodes rows): destination-major rows fo_fwd_ptr / fo_fwd_idx /
 * fo_fwd_val / fo_self of the owned nodes, source-major rows fo_shard_bwd_ptr [num_nodes + 1] (count phase) / _idx / _val [A1] — the successor
 * runs of ALL nodes that fall into the owned range (the out-lists of foreign nodes hold exactly their events into it). */
int pp_debruijn2_part_count(const int64_t* edge_index, const void* time, int time_dtype, int64_t m, int64_t num_nodes, int64_t node_lo, int64_t n_own,
                            const int64_t* cuts, int world, int rank, int delta_kind, int64_t delta_i, double delta_f, const float* weight,
                            int32_t* fo_bwd_ptr, int32_t* fo_bwd_idx, float* fo_w, int32_t* fo_fwd_ptr, int32_t* ho_fwd_ptr, int32_t* ho_bwd_ptr,
                            float* ho_deg, float* fo_deg, int32_t* send_slot, int32_t* row_of, int32_t* fo_shard_bwd_ptr, int64_t pad_rows,
                            int32_t* bip_fwd_ptr, int32_t* bip_fwd_idx, int32_t* bip_bwd_ptr, int32_t* bip_bwd_idx, float* bip_self, void* ws,
                            size_t ws_bytes, pp_stream_t stream);
int pp_debruijn2_part_fill(int time_dtype, int64_t m, int64_t num_nodes, int64_t node_lo, int64_t n_own, int delta_kind, int64_t delta_i, double delta_f,
                           const float* weight, const int32_t* fo_bwd_ptr, const int32_t* fo_fwd_ptr, const int32_t* ho_fwd_ptr,
                           const int32_t* ho_bwd_ptr, const float* ho_deg, const float* fo_deg, int64_t num_ho_edges, int32_t* ho_fwd_idx,
                           float* ho_fwd_val, int32_t* ho_bwd_idx, float* ho_bwd_val, float* ho_self, int32_t* fo_fwd_idx, float* fo_fwd_val,
                           float* fo_self, const int32_t* fo_shard_bwd_ptr, int32_t* fo_shard_bwd_idx, float* fo_shard_bwd_val, void* pair_scratch,
                           void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ all orders of a temporal stream, level by level (pp_multiorder.hip)
 *
 * MultiOrderModel.from_temporal_graph(g, delta, max_order >= 3), src/pathpyG/core/multi_order_model.py:124-192: lift_order_temporal
 * (algorithms/temporal.py:17-54) followed, per order, by iterate_lift_order (multi_order_model.py:83-122) = lift_order_edge_index(_weighted,
 * aggr="src") (algorithms/lift_order.py:48-106) + the node-sequence extension (:114) + aggregate_edge_index (lift_order.py:109-152).
 * The layers come out as source-major CSR (int32 row pointers / columns, float32 merged weights) — the reference's edge_index is
 * (row of every entry, column), its edge_weight the weights; neither the instance graphs [2, E_k] nor the [E_k, k] node sequences exist.
 *
 * A LEVEL k holds the order-(k+1) instances (time-respecting paths of k events) grouped by type (= edge of layer k = node of layer k+1),
 * types in lexicographic order:  tptr [types + 1] instance range of every type;  ibase [types + 1] first child of every type's instances
 * (ibase[types] = instances of level k+1);  col [types] column of the type in layer k;  tlast [types] its last node;
 * inst [instances] 16-byte records {window first, window count | head bit, last node, float32 weight of the first event}.
 *
 * pp_multiorder_prepare: level 1 from a finished pp_temporal_count or pp_temporal_windows (same stream, same delta; `lift_ws` is its workspace).  All outputs
 *   have capacity m (tptr / ibase: m + 1, rowptr: num_nodes + 1); `tab` [m] 16-byte records is the continuation table every step reads.
 *   Layer 1 = (rowptr, tlast as columns, w).  pp_multiorder_result_ptr(ws) = {types, status, instances of level 2 (= E2), long runs};
 *   status: bit 0 node index out of range, bit 1 time not ascending (both from pp_temporal_count).  The (source, target, time) order of the events:
 *   radix_sort == 0 sorts every node's time-ordered out-list (pp_temporal_count's) by target in LDS — no second global sort; a node with more than
 *   4096 out-events sets status bit 4 and leaves the outputs incomplete: call again with radix_sort != 0 (one stable radix sort of the stream by the
 *   (source, target) key).
 * pp_multiorder_step: level k+1 from level k.  cand_ptr / cand_last: row pointers of layer k (over ITS nodes) and the last nodes of
 *   level k's types (the candidates a column is looked up in; for k = 1: rowptr and tlast of pp_multiorder_prepare).  Outputs with capacity
 *   n_children (tptr_out / ibase_out: n_children + 1): child = inst of level k+1, row_ptr [n_types + 1] = row pointers of layer k+1,
 *   col_out / w_out = its columns and merged weights, tlast_out, tptr_out, ibase_out as above.  last != 0: the top layer — tptr_out,
 *   ibase_out, tlast_out are not written (may be NULL) and `child` is scratch of 4 (weighted: 8) bytes per child instead of 16.  weighted == 0: every event weighs 1 (merged weight = run length).
 *   pp_multiorder_result_ptr(ws) = {types of level k+1, status, instances of level k+2, types handled by workgroups};
 *   status bit 2: a type with more than 4096 children — the outputs are incomplete, use the generic kernels (pp_linegraph_*, pp_coalesce_*). */
size_t pp_multiorder_prepare_ws_bytes(int64_t m);
int pp_multiorder_prepare(const int64_t* edge_index, int64_t m, int64_t num_nodes, const float* weight, void* lift_ws, size_t lift_ws_bytes,
                          int radix_sort, void* tab, void* inst, int32_t* tptr, int32_t* ibase, int32_t* tlast, float* w, int32_t* rowptr, void* ws,
                          size_t ws_bytes, pp_stream_t stream);
/* The same from a GIVEN event graph (from_temporal_graph(..., event_graph=lift_order_temporal(g, delta)), multi_order_model.py:124-192 with
 * `event_graph` set): event_graph [2, num_event_edges] int64, sorted by source (as lift_order_temporal / lift_order_edge_index leave it; the order of
 * a source's targets is kept: it is the reference's instance order).  graph_ws: pp_multiorder_graph_ws_bytes; `tab` has num_event_edges records.
 * Status bit 0: an event id outside [0, m); bit 1: the event graph is not sorted by source. */
size_t pp_multiorder_graph_ws_bytes(int64_t m, int64_t num_event_edges);
int pp_multiorder_prepare_graph(const int64_t* edge_index, int64_t m, int64_t num_nodes, const float* weight, const int64_t* event_graph,
                                int64_t num_event_edges, void* graph_ws, size_t graph_ws_bytes, void* tab, void* inst, int32_t* tptr,
                                int32_t* ibase, int32_t* tlast, float* w, int32_t* rowptr, void* ws, size_t ws_bytes, pp_stream_t stream);
const int64_t* pp_multiorder_result_ptr(void* ws);
size_t pp_multiorder_step_ws_bytes(int64_t n_types, int64_t n_children);
int pp_multiorder_step(int64_t n_types, int64_t n_children, const int32_t* tptr, const int32_t* ibase, const int32_t* col, const void* inst,
                       const int32_t* cand_ptr, const int32_t* cand_last, const void* tab, int weighted, int last, void* child, int32_t* row_ptr,
                       int32_t* tptr_out, int32_t* ibase_out, int32_t* tlast_out, int32_t* col_out, float* w_out, void* ws, size_t ws_bytes,
                       pp_stream_t stream);
/* The same layers on N ranks, split by FIRST NODE (the reference builds them on one device only: MultiOrderModel.from_temporal_graph,
 * src/pathpyG/core/multi_order_model.py:124-192, per order iterate_lift_order :83-122).  Types are in lexicographic order of their node
 * sequences and a child keeps its parent's first node, so the rank that owns the first-order nodes [node_lo, node_hi) as first nodes owns a
 * contiguous block of types at every level = a contiguous block of rows of every layer.  The stream and pp_temporal_windows are replicated.
 *
 * pp_multiorder_node_loads: what the cuts are chosen from, right after pp_temporal_windows (`lift_ws`).  loads [2, num_nodes + 1] int64:
 *   loads[0][v] = out-events of the nodes below v (= v's first position in the source-grouped list), loads[1][v] = level-2 instances that
 *   start at a node below v (sum of their events' window counts); loads[.][num_nodes] are the totals.
 * pp_multiorder_prepare_range: pp_multiorder_prepare for the events whose source lies in [node_lo, node_hi) — the list positions
 *   [p_lo, p_lo + m_own) with p_lo = loads[0][node_lo], m_own = loads[0][node_hi] - p_lo > 0.  inst / tptr / ibase / tlast / w have capacity
 *   m_own (tptr / ibase: m_own + 1) and are numbered from 0 on the rank; rowptr [node_hi - node_lo + 1] is the owned slice of layer 1's row
 *   pointers as offsets into the rank's own edges; tlast holds global node ids; `tab` [m] covers the whole stream (children end anywhere).
 *   ws: pp_multiorder_prepare_range_ws_bytes(m, m_own); the result header and the status bits are pp_multiorder_prepare's, bit 4 = a node of
 *   the range with more than 4096 out-events: call again with radix_sort != 0 (one stable radix sort of the rank's events by (source, target)).
 *   With [0, num_nodes) the outputs are pp_multiorder_prepare's, bit for bit.
 * pp_multiorder_step then runs unchanged on a rank's types with tptr / ibase of the rank and col / cand_ptr / cand_last GLOBAL: it writes
 *   global columns.
 * pp_multiorder_stitch: cand_ptr [rows + 1] / cand_last [edges] of the next step from the all-gathered pieces, one launch.  `gathered` holds
 *   `world` blocks of `stride` int32; block r = the row pointers of rank r's rows (row_lo[r+1] - row_lo[r] entries, offsets into its own
 *   edges) and, from entry `last_at` on, the last nodes of its edges (edge_lo[r+1] - edge_lo[r] entries).  row_lo / edge_lo: HOST arrays
 *   [world + 1] of the ranks' first global row / edge, world <= 128.  cand_ptr[i] = piece entry + edge_lo[rank], cand_ptr[rows] = edges. */
size_t pp_multiorder_node_loads_ws_bytes(int64_t m);
int pp_multiorder_node_loads(int64_t m, int64_t num_nodes, void* lift_ws, size_t lift_ws_bytes, int64_t* loads, void* ws, size_t ws_bytes,
                             pp_stream_t stream);
size_t pp_multiorder_prepare_range_ws_bytes(int64_t m, int64_t m_own);
int pp_multiorder_prepare_range(const int64_t* edge_index, int64_t m, int64_t num_nodes, const float* weight, void* lift_ws, size_t lift_ws_bytes,
                                int64_t node_lo, int64_t node_hi, int64_t p_lo, int64_t m_own, int radix_sort, void* tab, void* inst, int32_t* tptr,
                                int32_t* ibase, int32_t* tlast, float* w, int32_t* rowptr, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_multiorder_stitch(const int32_t* gathered, int64_t stride, int64_t last_at, int world, const int64_t* row_lo, const int64_t* edge_lo,
                         int32_t* cand_ptr, int32_t* cand_last, pp_stream_t stream);
/* A level in PASSES on one GPU: a level with more children than int32 ids hold (or than a budget of the caller's) is cut into contiguous ranges
 * of whole types, pp_multiorder_step runs unchanged on one range after another (tptr / ibase of the range numbered from 0, col / cand_ptr /
 * cand_last / tab global), and the ranges' layer pieces are joined.  The reference has no such limit: its lifts are int64 throughout
 * (src/pathpyG/algorithms/lift_order.py:65,76).
 *
 * pp_multiorder_split: the cuts of a level of n_types types and the rebased arrays of all parts, one launch sequence, no read-back.  ibase
 *   [n_types + 1] may be WRAPPED (a level with 2^31 or more children: the scan stores the low 32 bits of int64 sums); every single count is
 *   below 2^31 (the step clamps and sets status bit 2 otherwise), so the counts are the unsigned differences of neighbouring entries and their
 *   prefix is taken in int64.  Greedy rule: a part that starts at type t0 ends before the first type t with prefix[t + 1] - prefix[t0] >
 *   budget, holds at least one type; a single type above the budget is a part of its own.  report: int64 [4 + 3 * (max_parts + 1)] =
 *   {parts, status, children of the level, children of the largest part}, then three rows of max_parts + 1 entries of which parts + 1 are
 *   written: first type of part p, children before it, instances before it (tptr there).  tptr_out / ibase_out: int32 [n_types + max_parts];
 *   part p's types_p + 1 entries start at entry (first type of p) + p.  max_parts <= min(n_types, 65536): one lane walks the cuts, a
 *   bisection per part; the split is meant for two to a few hundred parts.  status bit 0: more than max_parts parts (2 * children /
 *   budget + 2 always suffice: two neighbouring parts together exceed the budget); bit 1: a single type with 2^31 - 16 or more children; bit 2: ibase is
 *   not the low 32 bits of an ascending prefix of counts below 2^31.  With a bit set the rebased arrays are not written.
 *   ws: pp_multiorder_split_ws_bytes(n_types).
 * pp_multiorder_concat: n_pieces layer pieces in part order -> the layer's global arrays.  HOST arrays [n_pieces] of DEVICE pointers (as
 *   pp_adam_f32 takes its tensors) row_ptr (rows[k] entries are read: offsets into the piece's own edges), col, weight, last (edges[k]
 *   entries; `last` and last_out may be NULL: the top layer) and HOST arrays rows / edges.  row_ptr_out [sum rows + 1] = piece entry + the
 *   edges of the pieces before, closed by the edge total; col_out / weight_out / last_out [sum edges] the pieces' arrays one after another.
 *   A piece without edges has rows[k] empty rows; all its arrays, row_ptr included, may be NULL.  No staging copy; PP_ERR_TOO_LARGE at 2^31 - 16 rows or edges. */
size_t pp_multiorder_split_ws_bytes(int64_t n_types);
int pp_multiorder_split(int64_t n_types, const int32_t* tptr, const int32_t* ibase, int64_t budget, int64_t max_parts, int64_t* report,
                        int32_t* tptr_out, int32_t* ibase_out, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_multiorder_concat(int n_pieces, const void* const* row_ptr, const void* const* col, const void* const* weight, const void* const* last,
                         const int64_t* rows, const int64_t* edges, int32_t* row_ptr_out, int32_t* col_out, float* weight_out, int32_t* last_out,
                         pp_stream_t stream);
/* The same layers of OBSERVED WALKS: MultiOrderModel.from_path_data(paths, max_order >= 2, mode="propagation"),
 * src/pathpyG/core/multi_order_model.py:194-241, on the walk store of PathData.append_walks, src/pathpyG/core/path_data.py:126-159:
 * node_sequence [positions] int64 the first-order node of every walk position, dag_num_nodes [walks] int64 positions per walk (L_w >= 1),
 * dag_weight [walks] float32, edge_index [2, m] int64 the chain (p, p + 1) of the positions of every walk, m = positions - walks.
 * A position p of walk w(p) that is not its walk's last starts edge e = p - w(p) from node[p] to node[p + 1]; edge e continues into edge
 * e + 1 iff p + 1 is not the last position of its walk either.
 *
 * pp_multiorder_prepare_paths: level 1, the outputs of pp_multiorder_prepare (same capacities with m edges for m events; `tab` [m] is indexed
 *   by the edge id: {dst(e), e + 1, continues, e}), ready for pp_multiorder_step; the weight of an instance is its walk's dag_weight
 *   (lift_order_edge_index_weighted with aggr="src"), instances of a node pair in position order (one stable radix sort by (source, target)).
 *   edge_walk [m] int32: the walk of every edge (pp_multiorder_paths_inverse reads it).  ws: pp_multiorder_paths_ws_bytes(positions, walks,
 *   num_nodes); pp_multiorder_result_ptr(ws) = {types, status, instances of level 2, long runs}.  The walk store is verified on the device:
 *   status bit 3: the distinct node ids are not exactly 0 .. num_nodes - 1 (layer 1 of a path model uses the ids as given, lift_order.py:135-136;
 *     only id == rank is taken);
 *   status bit 5: edge_index is not the chain (p, p + 1) of these walks, some L_w < 1, or the L_w do not add up to `positions`;
 *   bit 2 as pp_multiorder_prepare.  With bit 3 or 5 set the outputs are not to be used (nothing was written out of bounds): the caller takes the
 *   generic kernels (pp_linegraph_*, pp_coalesce_*).
 * pp_multiorder_paths_inverse: inverse_idx of layer level + 1 (level >= 1) — for every (level + 1)-gram of consecutive walk positions, in
 *   start-position order (the reference's instance order), its node of layer level + 1 = its type at `level` — from that level while its
 *   `inst` is alive: tptr [n_types + 1], inst [n_instances] as pp_multiorder_prepare_paths (level 1) or pp_multiorder_step (child, last == 0)
 *   left them.  Instance i of type t ends with edge e = inst[i].x - 1, starts with f = e - (level - 1) and has the rank
 *   f - sum over the walks w' before edge_walk[e] of min(L_w' - 1, level - 1).  inverse [n_instances] int32.  ws: pp_multiorder_paths_inverse_ws_bytes(walks).
 * Known limit: a k-gram observed at more than 4096 walk positions that all continue is a type with more than 4096 children (status bit 2 of
 *   pp_multiorder_step): the whole model goes to the generic kernels, as on dense contact streams. */
size_t pp_multiorder_paths_ws_bytes(int64_t positions, int64_t walks, int64_t num_nodes);
int pp_multiorder_prepare_paths(const int64_t* node_sequence, int64_t positions, const int64_t* dag_num_nodes, const float* dag_weight, int64_t walks,
                                const int64_t* edge_index, int64_t m, int64_t num_nodes, void* tab, void* inst, int32_t* tptr, int32_t* ibase,
                                int32_t* tlast, float* w, int32_t* rowptr, int32_t* edge_walk, void* ws, size_t ws_bytes, pp_stream_t stream);
size_t pp_multiorder_paths_inverse_ws_bytes(int64_t walks);
int pp_multiorder_paths_inverse(int64_t level, int64_t n_types, int64_t n_instances, const int32_t* tptr, const void* inst, const int32_t* edge_walk,
                                int64_t m, const int64_t* dag_num_nodes, int64_t walks, int32_t* inverse, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ order lifts (pp_lift.hip) */

/* lift_order_temporal(g, delta) -> [2,E2] int64, src/pathpyG/algorithms/temporal.py:17-54.
 *   edge_index : [2,m] int64, events in time order (TemporalGraph.__init__ sorted them, temporal_graph.py:58-63)
 *   time       : [m] int64 (PP_I64) or float64 (PP_F64), ascending
 *   delta      : as torch.tensor(delta) sees it: PP_DELTA_I64 -> delta_i; PP_DELTA_F32 / PP_DELTA_F64 -> delta_f
 *                (for PP_DELTA_F32 pass the float32-rounded value).  With float64 time only delta_f is used.
 * pp_temporal_count builds the per-node event lists, counts each event's continuations and scans them;
 * pp_lift_result_ptr(ws)[0] = E2, [1] = status (bit 0: node index outside [0,num_nodes); bit 1: time is not ascending —
 * the result is then meaningless; the reference's mask-based loop has no such precondition, temporal.py:37-43).
 * pp_temporal_fill writes out[0][p] = i, out[1][p] = j for all pairs in lexicographic (i,j) order.
 * Edge-range sharding (one shard per GPU): pass the shard's events followed by its forward halo (all later events
 * with t <= t_last_owned + delta); only the first n_own events act as sources (n_own = m, or < 0, for the whole
 * stream) and id_offset (the global id of the shard's first event) is added to both rows of the result. */
size_t pp_temporal_ws_bytes(int64_t m, int64_t num_nodes);
int pp_temporal_count(const int64_t* edge_index, const void* time, int time_dtype, int64_t m, int64_t n_own, int64_t num_nodes,
                      int delta_kind, int64_t delta_i, double delta_f, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_temporal_fill(int64_t m, int64_t num_nodes, int64_t total, int64_t id_offset, int64_t* out, void* ws, size_t ws_bytes,
                     pp_stream_t stream);
/* Steps 1-2 of pp_temporal_count only — the per-node event lists and every event's continuation window, no output offsets (result[0] stays 0,
 * pp_temporal_fill must not follow): what pp_multiorder_prepare reads (the multi-order builder never writes the event graph). */
int pp_temporal_windows(const int64_t* edge_index, const void* time, int time_dtype, int64_t m, int64_t num_nodes, int delta_kind, int64_t delta_i,
                        double delta_f, void* ws, size_t ws_bytes, pp_stream_t stream);

/* lift_order_edge_index(edge_index, num_nodes) -> [2,E'] int64, src/pathpyG/algorithms/lift_order.py:48-79.
 * edge_index must be grouped by source like the reference demands (:52,55). */
size_t pp_linegraph_ws_bytes(int64_t n_edges, int64_t num_nodes);
int pp_linegraph_count(const int64_t* edge_index, int64_t n_edges, int64_t e_begin, int64_t e_end, int64_t num_nodes, void* ws,
                       size_t ws_bytes, pp_stream_t stream);   /* [e_begin, e_end): the source edges of this call (edge-range shard);
                                                                 out-degrees / row pointers always come from all n_edges edges */
int pp_linegraph_fill(int64_t n_edges, int64_t num_nodes, int64_t total, int64_t* out, void* ws, size_t ws_bytes, pp_stream_t stream);
const int64_t* pp_lift_result_ptr(void* ws); /* device pointer to {size, status} */

/* aggregate_node_attributes(edge_index, node_attribute, aggr), src/pathpyG/algorithms/lift_order.py:10-45.
 * attr is [num_nodes, width] row-major of `dtype`; out is [n_edges, width]; *status as above (device int64). */
int pp_edge_attr(const int64_t* edge_index, int64_t n_edges, const void* attr, int dtype, int64_t num_nodes, int64_t width, int aggr,
                 void* out, int64_t* status, pp_stream_t stream);

/* cat([ns[ei[0]], ns[ei[1]][:, -1:]], 1), src/pathpyG/core/multi_order_model.py:114,165: rows [n_rows,k] -> out [n_edges,k+1] */
int pp_extend_node_sequence(const int64_t* edge_index, int64_t n_edges, const int64_t* rows, int64_t n_rows, int k, int64_t* out,
                            int64_t* status, pp_stream_t stream);

/* out[i,:k] = rows[idx[i],:], out[i,k] = suffix[i]: the order-(k+1) node sequence of a node whose first k entries are the
 * order-k node idx[i] (multi_order_model.py:114 applied to DISTINCT nodes only, so instance sequences are never materialised) */
int pp_gather_concat(const int64_t* rows, int64_t n_rows, int k, const int64_t* idx, const int64_t* suffix, int64_t n, int64_t* out,
                     int64_t* status, pp_stream_t stream);

/* ------------------------------------------------------------------ De Bruijn aggregation (pp_aggregate.hip) */

/* torch.unique(node_sequence, dim=0, return_inverse=True), src/pathpyG/algorithms/lift_order.py:133.
 * rows [n_rows,k] int64 with every value in [min_value, max_value].  _count writes inverse[n_rows] and
 * {U, 0} to pp_aggregate_result_ptr(ws); _fill writes the U unique rows in lexicographic order. */
size_t pp_unique_rows_ws_bytes(int64_t n_rows);
int pp_unique_rows_count(const int64_t* rows, int64_t n_rows, int k, int64_t min_value, int64_t max_value, int64_t* inverse, void* ws,
                         size_t ws_bytes, pp_stream_t stream);
int pp_unique_rows_fill(const int64_t* rows, int64_t n_rows, int k, int64_t n_unique, int64_t* unique_rows, void* ws, size_t ws_bytes,
                        pp_stream_t stream);

/* coalesce(remap[edge_index], edge_attr, num_nodes, reduce), src/pathpyG/algorithms/lift_order.py:135-144.
 * remap may be NULL (edges already hold node ids).  _count -> {A, status}; _fill writes out_index [2,A]
 * sorted by (row, col) and the reduced weights (weight may be NULL; weight NULL with out_weight given = UNIT weights, the reference's
 * default `torch.ones` (lift_order.py:130-131): out_weight (float32 [A], whatever `dtype` says) = run length for sum, 1 otherwise, without the per-instance gather).
 * col_base [num_nodes] / col_bits (NULL / 0 = off; pass the same pair to _count and _fill): the caller knows that every column of row r
 * lies in [col_base[r], col_base[r] + 2^col_bits) - true for De Bruijn layers, where the successors of a node form one
 * contiguous id block - and the sort key shrinks from 2*bits(num_nodes) to bits(num_nodes) + col_bits bits (fewer radix passes);
 * an edge outside its block sets the bad-index status bit. */
size_t pp_coalesce_ws_bytes(int64_t n_edges);
int pp_coalesce_count(const int64_t* edge_index, int64_t n_edges, const int64_t* remap, int64_t remap_len, int64_t num_nodes,
                      const int64_t* col_base, int col_bits, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_coalesce_fill(const void* weight, int dtype, int reduce, int64_t n_edges, int64_t n_out, int64_t num_nodes, const int64_t* col_base,
                     int col_bits, int64_t* out_index,
                     void* out_weight, void* ws, size_t ws_bytes, pp_stream_t stream);
/* inverse[n_edges] = position of every input edge's merged edge (call between _count and the end of the workspace's life).
 * For a first-order event list this equals the inverse_idx of torch.unique over the (src,dst) rows, lift_order.py:133, i.e.
 * layer 2's node ids come for free from layer 1's coalesce. */
int pp_coalesce_inverse(int64_t n_edges, int64_t* inverse, void* ws, size_t ws_bytes, pp_stream_t stream);
const int64_t* pp_aggregate_result_ptr(void* ws);

/* Graph.__init__ helpers, src/pathpyG/core/graph.py:103-115 (EdgeIndex.sort_by("row"), get_csr, get_csc) */
int pp_count_descents_i64(const int64_t* a, int64_t n, int64_t* descents, pp_stream_t stream);
int pp_count_descents_f64(const double* a, int64_t n, int64_t* descents, pp_stream_t stream);
size_t pp_argsort_ws_bytes(int64_t n);
int pp_argsort_i64(const int64_t* keys, int64_t n, int64_t min_value, int64_t max_value, int64_t* perm_out, void* ws, size_t ws_bytes,
                   pp_stream_t stream);
/* stable replacement of torch.argsort(time) for float64 timestamps, src/pathpyG/core/temporal_graph.py:58.  The order of float64 values
 * here and in pp_count_descents_f64 / pp_time_stats / the sortedness checks of the temporal builders is torch.sort's: ascending,
 * -0.0 == 0.0, every NaN (either sign, any payload) after +inf and tied; a NaN directly before a number is a descent. */
int pp_argsort_f64(const double* keys, int64_t n, int64_t* perm_out, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_ptr_from_sorted_i64(const int64_t* sorted, int64_t n, int64_t num_rows, int64_t* ptr, pp_stream_t stream);
/* TemporalGraph.__init__, src/pathpyG/core/temporal_graph.py:58-63 (argsort of the timestamps, then edge_index / time indexed by it):
 * out3 = {descents, min, max} of the timestamps in one device buffer (float64: descents only) — one read-back says whether a sort is
 * needed and how many key bits it takes; pp_gather_events applies the permutation to the three 8-byte columns of every event in one
 * pass (time_dtype PP_I64 or PP_F64; status bit 1: permutation entry out of range). */
int pp_time_stats(const void* time, int time_dtype, int64_t n, int64_t* out3, pp_stream_t stream);
int pp_gather_events(const int64_t* edge_index, const void* time, const int64_t* perm, int64_t m, int64_t* edge_index_out, void* time_out,
                     int64_t* status, pp_stream_t stream);

/* ------------------------------------------------------------------ ingest of integer temporal edge lists (pp_ingest.hip) */

/* read_csv_temporal_graph, src/pathpyG/io/pandas.py:511-546 (pandas.read_csv of a `v<sep>w<sep>t` file), and the three columns
 * df_to_temporal_graph, src/pathpyG/io/pandas.py:318-397, takes from that frame — for files whose every non-blank line is exactly
 * `[0-9]{1,18} sep [0-9]{1,18} sep -?[0-9]{1,18}`, ended by "\n", "\r\n" or the end of the file (blank lines, empty or a lone "\r",
 * are skipped as pandas skips them; a header line is the caller's to cut off).  `bytes` is ONE CHUNK of the file on the device: it
 * starts at a line start, ends behind a '\n' or at the end of the file, and holds n_bytes < 2^31 bytes; no byte at or past n_bytes is
 * read.  `sep` is one ASCII byte other than a digit, '-', '\r' and '\n' (PP_ERR_ARG otherwise).
 *
 * pp_ingest_index writes the offset of the first byte of every non-blank line to line_start[0 .. min(n_lines, line_cap)) in file order
 * and leaves int64 {n_lines, status, smallest offending byte offset (INT64_MAX: none), 0} at the START of the workspace.
 * pp_ingest_parse takes that SAME workspace (it reads n_lines from it, so no read-back lies between the two calls), parses line i into
 * v[i], w[i], t[i] (each [line_cap]) and ORs what it finds into the status.  A status other than 0 means "this file does not qualify",
 * not an error: both calls still return PP_OK, the columns then hold unspecified values, and the caller gives the file to pandas.  One
 * 32-byte read-back per chunk says everything.  line_cap >= (n_bytes + 1) / 6 can never be exceeded by a qualifying chunk. */
enum pp_ingest_status {
    PP_INGEST_BAD_BYTE = 1,     /* a byte that is neither a digit, the separator, '-', '\r' nor '\n' */
    PP_INGEST_FIELD_COUNT = 2,  /* a line with fewer or more than three fields */
    PP_INGEST_TOKEN_LONG = 4,   /* more than 18 digits */
    PP_INGEST_TOKEN_EMPTY = 8,  /* an empty field, or a '-' without digits */
    PP_INGEST_MINUS = 16,       /* a '-' anywhere but in front of the third field */
    PP_INGEST_BAD_CR = 32,      /* a '\r' that does not stand directly before '\n' */
    PP_INGEST_NO_LINES = 64,    /* no non-blank line at all */
    PP_INGEST_LINE_CAP = 128,   /* more than line_cap lines */
    /* pp_ingest_tokens_* only */
    PP_INGEST_LEADING_ZERO = 256, /* a node token of two or more digits that starts with '0' ("007" and "7" are different node IDs) */
    PP_INGEST_BAD_WEIGHT = 512,   /* a weight token that is not (0|[1-9][0-9]*)(\.[0-9]+)? with at most 15 digits in total */
    PP_INGEST_TOKEN_CAP = 1024    /* more than token_cap tokens */
};
size_t pp_ingest_index_ws_bytes(int64_t n_bytes);
int pp_ingest_index(const uint8_t* bytes, int64_t n_bytes, int sep, int32_t* line_start, int64_t line_cap, void* ws, size_t ws_bytes,
                    pp_stream_t stream);
size_t pp_ingest_parse_ws_bytes(int64_t n_bytes); /* == pp_ingest_index_ws_bytes: the two calls share one workspace */
int pp_ingest_parse(const uint8_t* bytes, int64_t n_bytes, int sep, const int32_t* line_start, int64_t line_cap, int64_t* v, int64_t* w,
                    int64_t* t, void* ws, size_t ws_bytes, pp_stream_t stream);

/* read_csv_path_data, src/pathpyG/io/pandas.py:572-599 (csv.reader of an n-gram file, ast.literal_eval of every weight), and the walk
 * store PathData.append_walks, src/pathpyG/core/path_data.py:126-159, makes of it — for files whose every non-blank line is one walk of
 * integer node IDs, `node (sep node)*`, with `weight` != 0 followed by `sep weight`:
 *   node   : 0|[1-9][0-9]{0,17}                     (a leading zero disqualifies: to csv.reader "007" and "7" are different nodes)
 *   weight : (0|[1-9][0-9]*)(\.[0-9]+)? with at most 15 digits in total, no sign, no exponent.  Its value is (double)digits / 10^f
 *            (f fraction digits, both operands exact doubles, one IEEE division) rounded once to float32: bit for bit what
 *            torch.tensor([ast.literal_eval(token)], dtype=torch.float) holds.
 * Lines end with "\n", "\r\n" or the end of the file; blank lines are skipped, exactly as pp_ingest_index defines them.  A line has any
 * number of fields, so the TOKENS are indexed, not the lines: a token starts at the first byte of every non-blank line and behind
 * every separator byte.  `bytes`, `n_bytes`, `sep` and the chunk rules are those of pp_ingest_index.
 *
 * pp_ingest_tokens_index writes, in file order, token_start[t] (byte offset) and token_line[t] (rank of the token's line) for
 * t < min(n_tokens, token_cap), and line_first_token[l] (rank of line l's first token) for l < min(n_lines, line_cap) plus one closing
 * entry line_first_token[n_lines] = n_tokens (the array has line_cap + 1 entries).  It leaves int64 {n_lines, status, smallest
 * offending byte offset (INT64_MAX: none), n_tokens} at the START of the workspace.
 * pp_ingest_tokens_parse takes that SAME workspace (no read-back between the two calls) and parses one token per lane; a lane reads
 * no byte at or past the next token's start or n_bytes.  With `weight` != 0 the last token of line l becomes weights[l] and the others
 * nodes[t - l]; with `weight` == 0 every token is a node, nodes[t], and weights is not written.  lengths[l] = nodes of line l.
 * nodes has token_cap entries, lengths and weights line_cap.  As with pp_ingest_parse a status other than 0 means "this file does not
 * qualify" (both calls return PP_OK, the outputs are unspecified): an empty token, a trailing separator, a line of the weight alone,
 * any other byte (a '.' in a node token, a space, a quote, a sign, a letter) and a '\r' not directly before '\n' all set a bit.
 * token_cap = line_cap = n_bytes / 2 + 1 can never be exceeded by a qualifying chunk. */
size_t pp_ingest_tokens_ws_bytes(int64_t n_bytes);
int pp_ingest_tokens_index(const uint8_t* bytes, int64_t n_bytes, int sep, int32_t* token_start, int32_t* token_line, int64_t token_cap,
                           int32_t* line_first_token, int64_t line_cap, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_ingest_tokens_parse(const uint8_t* bytes, int64_t n_bytes, int sep, int weight, const int32_t* token_start,
                           const int32_t* token_line, int64_t token_cap, const int32_t* line_first_token, int64_t line_cap,
                           int64_t* nodes, int64_t* lengths, float* weights, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ DBGNN message passing (pp_dbgnn.hip) */

/* What PyG's gcn_norm computes on every GCNConv call of DBGNN.forward (src/pathpyG/nn/dbgnn.py:133,139):
 * add_remaining_self_loops(fill 1), weighted in-degree, d^-1/2, norm_e = d[row] w_e d[col] — built ONCE per graph:
 *   in_*  : CSR over DESTINATION nodes (in_ptr [N+1], in_idx = source of each incoming edge, in_val = norm)   forward
 *   out_* : CSR over SOURCE nodes      (out_idx = destination, out_val = norm)                               backward
 *   self_coef[i] = d[i]^2 * (weight of node i's self loop, 1 if it had none); existing self-loop edges get norm 0.
 * edge_weight may be NULL (all ones).  row_sorted != 0: the caller guarantees edge_index[0] is non-decreasing (every Graph's
 * edge index is, graph.py:103) and the source-major grouping reuses the edge order instead of sorting.
 * pp_plan_result_ptr(ws)[1] = status (bit 0: index out of range); [2] / [3] = longest row of the destination-major / source-major CSR (plans
 * with rows above a few hundred entries want pp_spmm_heavy_f32's chunk tables) — written by every plan builder below, one read-back for all. */
size_t pp_gcn_plan_ws_bytes(int64_t n_edges, int64_t n_nodes);
int pp_gcn_plan(const int64_t* edge_index, const float* edge_weight, int64_t n_edges, int64_t n_nodes, int row_sorted, int32_t* in_ptr,
                int32_t* in_idx, float* in_val, int32_t* out_ptr, int32_t* out_idx, float* out_val, float* self_coef, int32_t* dst_order,
                void* ws, size_t ws_bytes, pp_stream_t stream);   /* dst_order [E] or NULL: the edge ids grouped by destination (the
                                                                    permutation behind in_*); with in_ptr it IS the bipartite "last"
                                                                    plan of an order-2 model, whose nodes are this graph's edges */

/* The same plan for a DESTINATION-ROW PARTITION of the graph (multi-GPU DBGNN; the reference is single-process): this rank owns
 * n_dst destination rows; its local source space has n_src >= n_dst rows, the first n_dst being the owned nodes themselves (source i ==
 * destination i) and the rest halo rows owned by peers.  edge_index holds LOCAL ids (row 0 < n_src, row 1 < n_dst).  Two phases around
 * the one exchange the normalisation needs:
 *   pp_gcn_plan_begin : destination grouping, self loops, weighted in-degree -> dinv[0..n_dst), self_coef[n_dst]; with row_sorted
 *                       also out_ptr [n_src+1]
 *   (the caller fills dinv[n_dst..n_src) with the owners' values — one halo exchange of 4 bytes per halo row)
 *   pp_gcn_plan_finish: coefficients dinv[src] w dinv[dst] of both groupings (in_val in place; out_*).
 * The workspace (pp_gcn_plan_ws_bytes(n_edges, n_src)) carries the state between the two calls and must not be touched in between.
 * pp_gcn_plan == begin + finish with n_src == n_dst. */
int pp_gcn_plan_begin(const int64_t* edge_index, const float* edge_weight, int64_t n_edges, int64_t n_src, int64_t n_dst, int row_sorted,
                      int32_t* in_ptr, int32_t* in_idx, float* in_val, int32_t* out_ptr, float* self_coef, float* dinv, int32_t* dst_order,
                      void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_gcn_plan_finish(const int64_t* edge_index, const float* edge_weight, int64_t n_edges, int64_t n_src, int64_t n_dst, int row_sorted,
                       const float* dinv, const int32_t* in_idx, float* in_val, int32_t* out_ptr, int32_t* out_idx, float* out_val, void* ws,
                       size_t ws_bytes, pp_stream_t stream);

/* CSR views of DBGNN's bipartite_edge_index [2,n_pairs] (row 0: higher-order node, row 1: first-order node),
 * src/pathpyG/nn/dbgnn.py:64-69: in_* grouped by first-order node (+ its in-degree as float), out_* by higher-order node.
 * src_sorted != 0: row 0 is non-decreasing (arange for the reference's "last"/"first" mappings): no source-major sort.
 * pair_value (optional, with in_val/out_val): a coefficient per pair carried into both groupings — this makes the call a
 * general RECTANGULAR plan builder (sources x destinations), used for the destination-partitioned multi-GPU DBGNN where a rank
 * owns a slice of the destination rows but aggregates from all source rows.
 * Workspace: pp_gcn_plan_ws_bytes(n_pairs, max(n_ho, n_fo)). */
int pp_bipartite_plan(const int64_t* bipartite_index, int64_t n_pairs, int64_t n_ho, int64_t n_fo, int src_sorted, const float* pair_value,
                      int32_t* in_ptr, int32_t* in_idx, float* in_val, float* in_degree, int32_t* out_ptr, int32_t* out_idx, float* out_val,
                      void* ws, size_t ws_bytes, pp_stream_t stream);
const int64_t* pp_plan_result_ptr(void* ws);

/* Y[r,:] = act( sum_{p in [ptr[r],ptr[r+1])} val[p] * X[idx[p],:] + self_coef[r] * S[r,:] + bias ),  X:[*,F], Y:[n_rows,F] fp32.
 * val NULL = 1, self_coef NULL = no self term, S NULL = X, bias NULL = none, act 0 = identity / 1 = ELU.
 * GCNConv.propagate + bias + F.elu (dbgnn.py:133,139), the bipartite propagate + elu (:143-144) and all their transposes. */
int pp_spmm_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* X, int F, const float* self_coef,
                const float* S, const float* bias, int act, const int32_t* heavy_slot, const float* heavy_sum, float* Y, pp_stream_t stream);

/* Hub rows (scale-free graphs: 10^5+ entries in one CSR row).  The row kernels (pp_spmm_f32, pp_gcn_forward_f32, pp_gcn_backward_f32)
 * walk a row with ONE lane group; for rows the caller marks as heavy (heavy_slot [n_rows] int32: -1 = ordinary, else h) they read the
 * neighbour sum from heavy_sum [n_heavy, F] instead, which pp_spmm_heavy_f32 computes with a whole workgroup per chunk of
 * pp_heavy_chunk_entries() entries and a fixed-order combine (bit-reproducible).  heavy_slot NULL = no heavy rows.
 * pp_max_row_length_i32: out_max[0] (device int64) = longest row of a CSR pointer array, to decide whether a plan needs this. */
int pp_max_row_length_i32(const int32_t* ptr, int64_t n_rows, int64_t* out_max, pp_stream_t stream);
int pp_heavy_chunk_entries(void);
size_t pp_spmm_heavy_ws_bytes(int64_t n_chunks, int F);
int pp_spmm_heavy_f32(const int32_t* idx, const float* val, const float* X, int F, int64_t n_chunks, const int32_t* chunk_begin,
                      const int32_t* chunk_end, int64_t n_heavy, const int32_t* heavy_chunk_ptr, float* heavy_sum, void* ws, size_t ws_bytes,
                      pp_stream_t stream);

/* Transposed aggregation fused with the ELU backward of the layer that produced its input and with that layer's bias gradient:
 *   dX[r,:] = ( sum_{p in [ptr[r],ptr[r+1])} val[p] * D[idx[p],:] ) * ELU'(Z[r,:]),   colsum[F] (may be NULL) = column sums of dX
 * with Z the stored activation ELU(pre) and ELU' = (Z > 0 ? 1 : Z + 1).  F a multiple of 4, <= 256.  Used for the backward of the
 * bipartite aggregation sum_j x_h[j] (dbgnn.py:50-69 re-associated: lin1 is applied AFTER the sum over the higher-order nodes). */
int pp_spmm_act_backward_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* D, int F, const float* Z,
                             float* colsum, float* dX, pp_stream_t stream);
/* the same with Z stored DROPPED (F.dropout between the last higher-order layer and the bipartite layer, dbgnn.py:142; masks of pp_dropout_f32):
 * dX = (A D) * mask / (1 - p) * ELU'(Z * (1 - p)) */
int pp_spmm_act_backward_drop_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* D, int F, const float* Z,
                                  float* colsum, float* dX, double drop_p, int64_t drop_seed, int64_t drop_tag, int64_t drop_row0,
                                  pp_stream_t stream);

/* dpre = dY * elu'(.) from the stored OUTPUT y (1 if y > 0 else y + 1); act 0: dpre = dY; dbias[F] = column sums of dpre.
 * dpre or dbias may be NULL. */
int pp_act_backward_f32(const float* dY, const float* Y, int64_t n_rows, int F, int act, float* dpre, float* dbias, pp_stream_t stream);

/* The element-wise tail of BipartiteGraphOperator.forward + F.elu (src/pathpyG/nn/dbgnn.py:66-69,143-144) on the first-order rows, after the
 * re-association sum_j lin1(x_h[j]) = lin1.weight (sum_j x_h[j]) + deg * lin1.bias:  Y = ELU(A + deg[r] * (P + bias)),  A = lin1.weight applied
 * to the summed higher-order rows, P = lin2(x), deg [n_rows] = incoming pairs per first-order node, bias [F] or NULL.
 * _backward: dpre = dY * ELU'(Y);  dA = dpre;  dP = deg[r] * dpre;  dbias[c] = sum_r dP[r][c] (NULL: not wanted). */
int pp_bip_combine_f32(const float* A, const float* P, const float* deg, const float* bias, int64_t n_rows, int F, float* Y, pp_stream_t stream);
int pp_bip_combine_backward_f32(const float* dY, const float* Y, const float* deg, int64_t n_rows, int F, float* dA, float* dP, float* dbias,
                                pp_stream_t stream);

/* Partitioned DBGNN backward (no single-process counterpart in the reference; the sum it completes is the transposed aggregation of
 * GCNConv's backward, nn/dbgnn.py:131-140 under autograd): out[r,:] = own[r,:] + recv[slot[r],:] (slot[r] >= 0) + extra[r,:] + self_coef[r] * dpre[r,:],
 * every addend optional (NULL); recv/slot and self_coef/dpre come in pairs; F a multiple of 4, 16-byte aligned rows; out may alias own. */
int pp_halo_fold_f32(const float* own, const float* recv, const int32_t* slot, const float* extra, const float* self_coef, const float* dpre,
                     int64_t n_rows, int F, float* out, pp_stream_t stream);

/* out[r,:] = coef[r] * X[r,:] (gradient of the bipartite self term) */
int pp_scale_rows_f32(const float* X, const float* coef, int64_t n_rows, int F, float* out, pp_stream_t stream);

/* F.dropout(x, p, training=True) of DBGNN.forward (nn/dbgnn.py:132,136,138,142,148) with COUNTER-BASED masks: element (r, c) of a [n_rows, F] matrix
 * is kept iff hash(seed, tag, global row, c) >= p * 2^32 (two multiply-xorshift rounds on 32 bits), global row = rows[r] if rows != NULL else
 * row0 + r.  No mask tensor: the backward pass regenerates it, and the ranks of a partitioned run agree on every row.
 *   pp_dropout_f32               out = x * keep / (1 - p)                                   (out may alias x)
 *   pp_dropout_act_backward_f32  dpre = dY * keep / (1 - p) * (act ? ELU'(y) : 1), y = Ydrop * (1 - p) where kept;  dbias[F] (optional) = column sums
 * i.e. the backward of dropout and the ELU backward of the layer underneath in one pass over (dY, Ydrop). */
int pp_dropout_f32(const float* X, int64_t n_rows, int F, double p, int64_t seed, int64_t tag, int64_t row0, const int64_t* rows, float* out,
                   pp_stream_t stream);
int pp_dropout_act_backward_f32(const float* dY, const float* Ydrop, int64_t n_rows, int F, double p, int64_t seed, int64_t tag, int64_t row0,
                                const int64_t* rows, int act, float* dpre, float* dbias, pp_stream_t stream);

/* F.dropout of the DEFAULT one-hot features (torch.eye, core/multi_order_model.py:529-533; dropped at nn/dbgnn.py:132,136) without the
 * identity: dropout keeps or drops only the diagonal of I, so dropout(I) W^T = diag(d) W^T with d[g] = the factor pp_dropout_f32 gives element
 * (g, g) of an [n, n] matrix (hash index g * n + g; 0 or 1 / (1 - p)).  out[r,:] = X[r,:] * d[row0 + r] for an [n_rows, F] matrix whose rows are
 * the rows row0 .. row0 + n_rows of that product (forward: X = W^T; backward: X = A_hat^T dpre, out = dW^T).  Any F; out may alias X. */
int pp_dropout_diag_rows_f32(const float* X, int64_t n_rows, int F, int64_t n, double p, int64_t seed, int64_t tag, int64_t row0, float* out,
                             pp_stream_t stream);
/* The first GCN layer on those features (GCNConv + F.elu on dropout(torch.eye), nn/dbgnn.py:132-133,136-137; core/multi_order_model.py:529-533)
 * with the factor inside the aggregation — pp_spmm_f32 (S = X, no hub rows) with d as above for rows 0 .. n:
 *   where 1 (forward)   Y[r,:] = act( sum_p val[p] * d[idx[p]] * X[idx[p],:] + self_coef[r] * d[r] * X[r,:] + bias ),  X = W^T: no scaled copy
 *   where 2 (backward)  Y[r,:] = d[r] * ( sum_p val[p] * X[idx[p],:] + self_coef[r] * X[r,:] ),  X = dpre over the transposed CSR, Y = dW^T
 * F a multiple of 4 in [4, 256], 16-byte aligned rows, n_rows <= n; self_coef NULL = no self term. */
int pp_spmm_diag_drop_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, const float* X, int F, const float* self_coef,
                          const float* bias, int act, int where, int64_t n, double p, int64_t seed, int64_t tag, float* Y, pp_stream_t stream);
/* The same layer (nn/dbgnn.py:132-133,136-137 on the default features of core/multi_order_model.py:529-533) on ONE RANK's share of a
 * destination-row partition: the CSR runs over LOCAL slots [owned | halo] and map[slot] (int64, distinct values in [0, n)) is the global id g,
 * at which d[g] is hashed and the replicated matrix W^T [n, F] is addressed — no feature row is stored or exchanged for such a graph.
 *   where 1 (forward)   Y[r,:] = act( sum_p val[p] * d[map[idx[p]]] * X[map[idx[p]],:] + self_coef[r] * d[map[r]] * X[map[r],:] + bias ),
 *                       r < n_rows = n_self owned rows, X = W^T [n, F], Y [n_rows, F]
 *   where 2 (backward)  Y[map[s],:] = d[map[s]] * ( sum_p val[p] * X[idx[p],:] + (s < n_self ? self_coef[s] * X[s,:] : 0) ),  s < n_rows local
 *                       source slots over the transposed CSR, X = dpre [n_self, F], Y [n, F] = the rank's partial dW^T, zero-filled by the
 *                       CALLER (rows of ids no slot maps to are not written); plain stores, the ids are distinct.
 * CSR-entry order and additions are pp_spmm_diag_drop_f32's: with map = 0 .. n_rows the results are the same bits.  Conditions as there. */
int pp_spmm_diag_drop_map_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, const float* X, int F,
                              const float* self_coef, const float* bias, int act, int where, const int64_t* map, int64_t n, double p, int64_t seed,
                              int64_t tag, float* Y, pp_stream_t stream);

/* Weight gradient of a dense layer of the DBGNN (autograd of lin / lin1 / lin2 / GCNConv.lin, dbgnn.py:64,133,139,149):
 * dW[M,K] = dH[N,M]^T X[N,K] and, when db != NULL, db[M] = column sums of dH.  fp32 on the matrix cores
 * (v_mfma_f32_32x32x2_f32, operands read straight from the row-major inputs), deterministic two-stage reduction. */
size_t pp_weight_grad_ws_bytes(int64_t n_rows, int M, int K);
int pp_weight_grad_f32(const float* dH, const float* X, int64_t n_rows, int M, int K, float* dW, float* db, void* ws, size_t ws_bytes,
                       pp_stream_t stream);

/* Dense layer on the matrix cores (the Linear / GCNConv.lin calls of dbgnn.py:64,133,139,149 and their input gradients):
 *   out[N,Q] = ( A[N,P] . B + bias ) (*) g'      B = W^T for w_transposed != 0 (W is [Q,P]: forward), W otherwise (W is [P,Q])
 *   grad_act : [N,Q] or NULL: the stored activation y = ELU(pre) of the layer below; the result is multiplied by
 *              ELU'(pre) = (y > 0 ? 1 : y + 1) and, with colsum [Q], its column sums (= that layer's bias gradient) accumulate.
 * fp32 on v_mfma_f32_16x16x4_f32.  pp_dense_supported(P, Q): 1 = P, Q in {16, 32, 64} (weights in registers; also pp_dense_backward_f32),
 * 2 = other widths whose padded product is <= 4096, e.g. anything up to 64 x 64 or 256 x 8 (zero-padded: pp_dense_narrow_f32), 3 = 64/128/256 with a side > 64 (pp_wide_layer_f32 in dense mode; with
 * w_transposed == 0 it needs ws = pp_wide_layer_ws_bytes(P, Q) bytes), 0 = not supported (the Python side then uses the library GEMM). */
int pp_dense_supported(int P, int Q);
int pp_dense_f32(const float* A, const float* W, int w_transposed, int64_t n_rows, int P, int Q, const float* bias,
                 const float* grad_act, float* colsum, float* out, void* ws, size_t ws_bytes, pp_stream_t stream);

/* Mean softmax cross-entropy of logits [n,C] (C <= 64) against int64 targets [n] and its gradient dlogits [n,C] (may be NULL) in
 * one pass - the loss of the train step bench.py times (the reference ships no training loop).  Per row, with m = z[a] the
 * row maximum:  loss_i = (m - z[y]) + log1p(sum_{c != a} exp(z[c] - m))  - F.cross_entropy's value without the saturation of
 * -log(softmax[y]) at large spreads and without the cancellation of m + log(sum) - z[y] on confident rows; a target on a class masked
 * with -inf gives +inf, and dlogits is exactly 0 in masked columns. */
size_t pp_cross_entropy_ws_bytes(void);       /* per-workgroup partial sums, added in a fixed order: the loss is bitwise reproducible */
int pp_cross_entropy_f32(const float* logits, const int64_t* target, int64_t n, int C, float* loss, float* dlogits, void* ws, size_t ws_bytes,
                         pp_stream_t stream);

/* The same loss over a SELECTION of the rows, with class weights - the objective of a semi-supervised node classifier (the reference's
 * tutorial loop trains on out[train_mask], docs/tutorial/netzschleuder.ipynb cells 15-17) without the boolean-index gather, its nonzero
 * read-back and the index_put backward.  Row i is selected iff (mask == NULL or mask[i] != 0) and (use_ignore == 0 or
 * target[i] != ignore_index); mask holds one byte per row, weight [C] fp32 may be NULL (all ones).
 *   dlogits_raw [n,C] (may be NULL) = w[y_i] (softmax(z_i) - onehot(y_i)) on selected rows, exactly 0.0f on every other row: the
 *                gradient of the SUM reduction; the mean's is dlogits_raw * inv_den.
 *   result     : 32 bytes on the device, 8-byte aligned: float num = sum w[y_i] nll_i, float den = sum w[y_i], float mean = num / den (NaN on
 *                an empty selection), float inv_den = 1 / den (0 when no valid row is selected), int64 selected rows, int64 selected
 *                rows whose target lies outside [0, C).
 * A selected row with an out-of-range target contributes nothing and gets a zero gradient row; no target is used as an index before that
 * test, unselected rows may hold any target and their logits are not loaded.  Per-row arithmetic as pp_cross_entropy_f32.  No float atomics:
 * per-workgroup partials (ws) are added in a fixed order, the same inputs give the same bits on every call; dlogits_raw does not depend on
 * the grid at all.  The grid follows pp_set_launch_share. */
size_t pp_cross_entropy_masked_ws_bytes(void);
int pp_cross_entropy_masked_f32(const float* logits, const int64_t* target, const uint8_t* mask, const float* weight, int64_t n, int C,
                                int64_t ignore_index, int use_ignore, void* result, float* dlogits_raw, void* ws, size_t ws_bytes, pp_stream_t stream);
/* The same pass for ONE RANK of a partitioned model (the tutorial loop of docs/tutorial/netzschleuder.ipynb cells 15-17 over rows that live on
 * several GPUs): raw_sums = 32 bytes on the device, 8-byte aligned: double num, double den, int64 selected, int64 out of range — the sums
 * BEFORE the rounding to fp32, so that the ranks' sums can be added (all-reduce) and rounded once.  dlogits_raw, ws as above. */
int pp_cross_entropy_masked_sums_f32(const float* logits, const int64_t* target, const uint8_t* mask, const float* weight, int64_t n, int C,
                                     int64_t ignore_index, int use_ignore, void* raw_sums, float* dlogits_raw, void* ws, size_t ws_bytes,
                                     pp_stream_t stream);
/* ... and the finish on the reduced sums: sums [2] double {num, den}, counts [2] int64 {selected, out of range} -> result, the 32 bytes of
 * pp_cross_entropy_masked_f32 with exactly its arithmetic (mean = (float)(num / den), inv_den = valid rows ? (float)(1 / den) : 0). */
int pp_masked_finish_f32(const double* sums, const int64_t* counts, void* result, pp_stream_t stream);

/* Confusion matrix of the predictions under the same selection: counts [C,C] int64 (zeroed by the callee), row = true class, column =
 * predicted class = the lowest column holding the row maximum, a NaN counting as the maximum (numpy's argmax).  status [1] int64 (zeroed by
 * the callee) = selected rows skipped because their target lies outside [0, C).  Per-workgroup histograms in LDS, flushed with integer
 * atomics: the result does not depend on the order.  1 <= C <= 64. */
int pp_confusion_f32(const float* logits, const int64_t* target, const uint8_t* mask, int64_t n, int C, int64_t ignore_index, int use_ignore,
                     int64_t* counts, int64_t* status, pp_stream_t stream);

/* One Adam step (step = 1, 2, ...) over ALL n_tensors fp32 parameter tensors in one launch per 24 tensors: HOST arrays of DEVICE pointers
 * (params, grads, exp_avg, exp_avg_sq) and of element counts.  The update of torch.optim.Adam (amsgrad off, maximize off; weight_decay is
 * the L2 form g + wd*p).  No reference counterpart: pathpyG ships the model (nn/dbgnn.py:72-151); its only training loop is the upstream tutorial
 * docs/tutorial/dbgnn.ipynb, which is absent from /root/reference (.MISSING_LARGE_BLOBS:2).  This is the optimizer step such a loop takes from
 * torch.optim.Adam (15 small launches there, one here). */
int pp_adam_f32(int n_tensors, void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel,
                double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, pp_stream_t stream);

/* Whole backward of a dense layer y = x W^T (+ b) in one pass over dH [N,M] and x [N,K] (W is [M,K]; M, K in {16,32,64}):
 *   d_in[N,K] = (dH . W) (*) ELU'(x) when fuse_act (x is then the stored activation of the layer below), colsum_in[K] = its column
 *   sums (that layer's bias gradient); dW[M,K] = dH^T x; db[M] = column sums of dH.  d_in/colsum_in/db may be NULL.
 * Replaces pp_dense_f32(input gradient) + pp_weight_grad_f32: 3 instead of 5 passes over N x 64 matrices. */
size_t pp_dense_backward_ws_bytes(int64_t n_rows);
int pp_dense_backward_f32(const float* dH, const float* X, const float* W, int64_t n_rows, int M, int K, int fuse_act, float* d_in,
                          float* colsum_in, float* dW, float* db, void* ws, size_t ws_bytes, pp_stream_t stream);

/* A whole GCNConv layer (dbgnn.py:131-140) in one kernel, re-associated as (A_hat X) W^T so that the transformed matrix never
 * makes a round trip through HBM:
 *   Y[r, :Q] = act( (sum_e val[e] X[idx[e], :P] + self_coef[r] X[r, :P]) . W^T + bias ),   W is [Q,P] (Linear layout), act 0/1 (ELU)
 * over the destination-major CSR of a pp_gcn_plan (self_coef may be NULL: no self term); X has n_src rows (rows are addressed by
 * 32-bit byte offsets below 4 GiB, by 64-bit ones above).  P, Q in {16,32,64}; the 128-wide shapes 64x128, 128x64, 128x128 (W then
 * fills 32-64 KB of LDS: one workgroup of 8 waves per CU); every other combination of 64/128/256 goes to pp_wide_layer_f32 (weights
 * streamed through LDS).  pp_gcn_fused_supported(P, Q): 1 = forward + pp_gcn_backward_f32, 2 = forward + pp_gcn_input_grad_f32
 * (a side of 128 or 256), 0 = unsupported shape.
 * agg_out [n_rows,P] or NULL: also store the aggregated input A_hat X; the weight gradient of a layer whose input needs no
 * gradient is then dW = dpre^T agg_out (pp_weight_grad_f32) without any backward aggregation. */
int pp_gcn_fused_supported(int P, int Q);
int pp_gcn_forward_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_src, const float* X, int P,
                       const float* self_coef, const float* W, int Q, const float* bias, int act, const int32_t* heavy_slot, const float* heavy_sum,
                       float* agg_out, float* Y, pp_stream_t stream);

/* Backward of that layer in one kernel (pp_spmm_f32 over the source-major CSR + pp_dense_backward_f32 without the round trip of the
 * aggregated gradient through HBM):  G = A^T D + diag(self_coef) D with D = dpre [n_rows,M];
 *   d_in[n_rows,K] = (G . W) (*) ELU'(X) when fuse_act (X [n_rows,K] is then the stored activation of the layer below),
 *   colsum_in[K] (may be NULL) = column sums of d_in,  dW[M,K] = G^T X.   W is [M,K]; M, K in {16,32,64}.
 * n_self <= n_rows: only the first n_self rows carry the self term (D then has n_self rows).  n_self == n_rows for a whole graph;
 * a destination-row partition (multi-GPU) has n_rows = owned + halo source rows and n_self = owned rows. */
size_t pp_gcn_backward_ws_bytes(int64_t n_rows);
int pp_gcn_backward_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, const float* D, int M,
                        const float* self_coef, const float* X, int K, const float* W, int fuse_act, const int32_t* heavy_slot,
                        const float* heavy_sum, float* d_in, float* colsum_in, float* dW, void* ws, size_t ws_bytes, pp_stream_t stream);

/* Input gradient of a 128-wide fused layer (GCNConv backward, reference nn/dbgnn.py:131-140 through autograd): the forward kernel over the
 * source-major CSR with a gradient epilogue,  d_in[n_rows,K] = ((A^T D + diag(self_coef) D) . W) (*) ELU'(X_act) when fuse_act,
 * colsum_in[K] (may be NULL) = column sums of d_in.  D = dpre [n_rows,M], W [M,K]; shapes 64x128, 128x64, 128x128.  The weight gradient
 * of such a layer is dW = dpre^T (A_hat X) with the agg_out of its forward call (pp_weight_grad_f32): 64 accumulator registers per
 * 64x64 block do not fit beside the gather here. */
int pp_gcn_input_grad_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, const float* D, int M,
                          const float* self_coef, const float* W, int K, const float* X_act, int fuse_act, const int32_t* heavy_slot,
                          const float* heavy_sum, float* d_in, float* colsum_in, void* ws, size_t ws_bytes, pp_stream_t stream);
/* The same three calls with the reference's training-mode F.dropout (src/pathpyG/nn/dbgnn.py:132,138,142) fused into their epilogues
 * (counter-based masks, see pp_dropout_f32; drop_p == 0: exactly the calls above; pp_gcn_drop_supported(P, Q): the 16/32/64 and 128-wide
 * kernels).  forward: Y is dropped — mask(drop_seed, drop_tag, drop_row0 + row, column) — before it is stored, i.e. the NEXT layer's input
 * dropout costs no pass.  backward / input_grad (with fuse_act): X / X_act is the dropped activation of the layer below (site drop_tag);
 * d_in becomes the gradient w.r.t. that layer's pre-activation, (G W) * mask / (1 - p) * ELU'(X * (1 - p)). */
int pp_gcn_drop_supported(int P, int Q);
int pp_gcn_forward_drop_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_src, const float* X, int P,
                            const float* self_coef, const float* W, int Q, const float* bias, int act, const int32_t* heavy_slot,
                            const float* heavy_sum, float* agg_out, float* Y, double drop_p, int64_t drop_seed, int64_t drop_tag, int64_t drop_row0,
                            pp_stream_t stream);
int pp_gcn_backward_drop_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, const float* D, int M,
                             const float* self_coef, const float* X, int K, const float* W, int fuse_act, const int32_t* heavy_slot,
                             const float* heavy_sum, float* d_in, float* colsum_in, float* dW, void* ws, size_t ws_bytes, double drop_p,
                             int64_t drop_seed, int64_t drop_tag, int64_t drop_row0, pp_stream_t stream);
/* The same call with the number of CSR entries, when the caller knows it (nnz < 0: unknown): graphs with short rows (nnz <= 8 n_rows, a
 * De Bruijn layer) run a register-capped variant of the 64 x 64 kernel (3 waves per SIMD); long-row graphs keep the 2-wave one. */
int pp_gcn_backward_nnz_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, int64_t nnz, const float* D, int M,
                            const float* self_coef, const float* X, int K, const float* W, int fuse_act, const int32_t* heavy_slot,
                            const float* heavy_sum, float* d_in, float* colsum_in, float* dW, void* ws, size_t ws_bytes, double drop_p,
                            int64_t drop_seed, int64_t drop_tag, int64_t drop_row0, pp_stream_t stream);
int pp_gcn_input_grad_drop_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, const float* D, int M,
                               const float* self_coef, const float* W, int K, const float* X_act, int fuse_act, const int32_t* heavy_slot,
                               const float* heavy_sum, float* d_in, float* colsum_in, void* ws, size_t ws_bytes, double drop_p, int64_t drop_seed,
                               int64_t drop_tag, int64_t drop_row0, pp_stream_t stream);
/* pp_gcn_backward_nnz_f32 of the SECOND layer of a stack whose first layer's input takes no gradient (the stacks of reference
 * src/pathpyG/nn/dbgnn.py:131-140: x and x_h are data): d_in, the gradient w.r.t. the first layer's pre-activation, is consumed where it is
 * formed —  dW_below[K,K_below] = d_in^T agg_below  with agg_below [n_rows,K_below] the agg_out of the first layer's forward call — and never
 * stored (d_in is ignored and may be NULL).  Replaces pp_gcn_backward_nnz_f32 + pp_weight_grad_f32: one write and one read of an
 * n_rows x 64 matrix and one launch less.  colsum_in and dW as above.  One variant only; PP_ERR_ARG unless M == K == K_below == 64,
 * fuse_act, colsum_in != NULL, n_self == n_rows, heavy_slot == NULL, drop_p == 0 and the matrices fit 32-bit byte offsets.
 * ws: pp_gcn_backward_below_ws_bytes(n_rows) (two sets of partial tiles). */
size_t pp_gcn_backward_below_ws_bytes(int64_t n_rows);
int pp_gcn_backward_below_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, int64_t nnz, const float* D, int M,
                              const float* self_coef, const float* X, int K, const float* W, int fuse_act, const int32_t* heavy_slot,
                              const float* heavy_sum, float* d_in, float* colsum_in, float* dW, void* ws, size_t ws_bytes, double drop_p,
                              int64_t drop_seed, int64_t drop_tag, int64_t drop_row0, const float* agg_below, int K_below, float* dW_below,
                              pp_stream_t stream);

                          /* ws: pp_wide_layer_ws_bytes(M, K) for the shapes served by pp_wide_layer_f32 (a side of 256), else unused */

/* Layers too wide for a weight matrix in LDS (pp_gcn_wide.hip): P, Q in {64, 128, 256} with a side > 64 — DBGNN with 256-dim features
 * (BASELINE configs[4]; GCNConv / Linear of nn/dbgnn.py:104-119 and their backward).  One kernel per layer:
 *   Y[n, :Q] = epi( tile[n, :P] . B ),  tile[n] = sum_e val[e] X[idx[e]] + self_coef[n] X[n]  (rows >= n_self: no self term)
 *                                       or X[n] when ptr == NULL (a dense layer; idx/val/self_coef ignored)
 *   B = W^T with W [Q,P] (w_is_kq == 0: Linear layout, the forward) or B = W with W [P,Q] (w_is_kq == 1: the input gradient; transposed
 *   once into ws, pp_wide_layer_ws_bytes(P, Q) bytes)
 *   epilogue 0: Y = act(.. + bias), agg_out [n_rows,P] (optional) receives the aggregated tile;
 *   epilogue 1: Y = (..) (*) ELU'(act_in) when act (act_in [n_rows,Q] = stored activation), colsum[Q] (optional) = column sums of Y.
 * The 16 x P tile lives in registers in MFMA A layout, the weights stream through LDS 16 output columns at a time. */
int pp_wide_layer_supported(int P, int Q);
size_t pp_wide_layer_ws_bytes(int P, int Q);
int pp_wide_layer_f32(const int32_t* ptr, const int32_t* idx, const float* val, int64_t n_rows, int64_t n_self, int64_t n_src, const float* X, int P,
                      const float* self_coef, const float* W, int w_is_kq, int Q, const float* bias, int act, int epilogue, const float* act_in,
                      const int32_t* heavy_slot, const float* heavy_sum, float* agg_out, float* Y, float* colsum, void* ws, size_t ws_bytes,
                      pp_stream_t stream);

/* Dense layers with one small side (classifier head: 64 -> 8 or 256 -> 8 classes and its input gradient; odd hidden widths): the
 * pp_dense_f32 scheme with both sides zero-padded to 16/32/64/128/256 (padded P*Q <= 4096) and guarded scalar I/O on the true widths.
 * Same arguments as pp_dense_f32. */
int pp_dense_narrow_supported(int P, int Q);
int pp_dense_narrow_f32(const float* A, const float* W, int w_transposed, int64_t n_rows, int P, int Q, const float* bias, const float* grad_act,
                        float* colsum, float* out, pp_stream_t stream);

/* The head of the DBGNN on the first-order rows (pp_head.hip): everything between the bipartite sum and the bipartite backward —
 * BipartiteGraphOperator after the re-association of lin1, its ELU and the classifier (reference nn/dbgnn.py:66-69,143-151):
 *   z      = ELU( agg . W1^T + deg (*) (x . W2^T + b2 + b1) )     agg [n,Ha] = summed higher-order rows, x [n,Hx] = stored ELU activation of the
 *   logits = z . Wlin^T + blin                                    first-order stack, deg [n] = bipartite in-degree; W1 [Hb,Ha], W2 [Hb,Hx], Wlin [C,Hb]
 * in ONE kernel (z [n,Hb] is stored for the backward, logits [n,C]); the products agg . W1^T and x . W2^T and the pre-activation never
 * reach memory.  pp_dbgnn_head_supported: Ha, Hx, Hb in {16, 32, 64} and 1 <= C <= 16; anything else is PP_ERR_ARG. */
int pp_dbgnn_head_supported(int Ha, int Hx, int Hb, int C);
int pp_dbgnn_head_forward_f32(const float* agg, const float* x, const float* deg, const float* W1, const float* b1, const float* W2, const float* b2,
                              const float* Wlin, const float* blin, int64_t n_rows, int Ha, int Hx, int Hb, int C, float* z, float* logits,
                              pp_stream_t stream);
/* Its backward (autograd of the same lines), per 16-row tile in registers:  dz = dlogits . Wlin,  dpre = dz (*) ELU'(z),  dper = deg (*) dpre,
 *   d_agg [n,Ha]   = dpre . W1                        (gradient of the bipartite sum)
 *   dpre_fo [n,Hx] = (dper . W2) (*) ELU'(x)          (gradient w.r.t. the PRE-activation of the first-order stack's last layer, as the
 *   colsum_fo [Hx] = column sums of dpre_fo            gradient epilogue of pp_dense_f32 / pp_dense_backward_f32 hands it down; = that layer's bias gradient)
 *   dW1 [Hb,Ha] = dpre^T agg,  dW2 [Hb,Hx] = dper^T x,  db1 = db2 [Hb] = column sums of dper,  dWlin [C,Hb] = dlogits^T z,  dblin [C] = column sums of dlogits.
 * dz, dpre and dper never reach memory.  The weight gradients are per-workgroup partial tiles summed in a fixed order (as pp_dense_backward_f32);
 * ws: pp_dbgnn_head_backward_ws_bytes(n_rows). */
size_t pp_dbgnn_head_backward_ws_bytes(int64_t n_rows);
int pp_dbgnn_head_backward_f32(const float* dlogits, const float* z, const float* agg, const float* x, const float* deg, const float* W1,
                               const float* W2, const float* Wlin, int64_t n_rows, int Ha, int Hx, int Hb, int C, float* d_agg,
                               float* dpre_fo, float* colsum_fo, float* dW1, float* dW2, float* db1, float* db2, float* dWlin, float* dblin,
                               void* ws, size_t ws_bytes, pp_stream_t stream);

/* All-pairs shortest time-respecting paths (temporal_shortest_paths, src/pathpyG/algorithms/temporal.py:57-107: scipy Dijkstra with
 * unit weights on the event DAG augmented by a virtual source and sink per node) as a frontier BFS per source node on the event graph:
 *   edge_index [2,m] time-sorted events;  succ_ptr [m+1] / succ [E2]: CSR of lift_order_temporal's result (row i -> events j);
 *   by_src_ptr [n+1] / by_src [m]: event ids grouped by their source node;
 *   dist [n,n] int32: number of events on a shortest path, -1 = unreachable, 0 on the diagonal;
 *   pred [n,n] int64: source node of the latest event that completes a shortest path into the column node (-1 none, s on the diagonal). */
size_t pp_temporal_bfs_ws_bytes(int64_t m, int64_t n);
int pp_temporal_bfs(const int64_t* edge_index, int64_t m, int64_t n, const int64_t* succ_ptr, const int64_t* succ, const int64_t* by_src_ptr,
                    const int64_t* by_src, int32_t* dist, int64_t* pred, void* ws, size_t ws_bytes, pp_stream_t stream);

/* Temporal betweenness centrality (temporal_betweenness_centrality, src/pathpyG/algorithms/centrality.py:164-297: Brandes on the event
 * DAG) in level-synchronous form, one workgroup per source node.  Inputs as pp_temporal_bfs plus the events grouped by their head
 * node (by_dst_ptr [n+1] / by_dst [m]).  partial [pp_temporal_betweenness_parts(m,n), n] float64: one row per workgroup; the
 * centrality of node v is the sum of column v over the rows (summed by the caller in row order: bit-reproducible while every path count
 * stays below 2^53, where the float64 counts are exact; within summation rounding up to 2^1024; from there on a count is inf, as the
 * reference's float counts are, and a ratio inf / inf counts as 0.0, the reference's isnan guard, centrality.py:282-289). */
int64_t pp_temporal_betweenness_parts(int64_t m, int64_t n);
size_t pp_temporal_betweenness_ws_bytes(int64_t m, int64_t n);
int pp_temporal_betweenness(const int64_t* edge_index, int64_t m, int64_t n, const int64_t* succ_ptr, const int64_t* succ,
                            const int64_t* by_src_ptr, const int64_t* by_src, const int64_t* by_dst_ptr, const int64_t* by_dst,
                            double* partial, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ static shortest paths and centralities (pp_graph_paths.hip) */
/* Unit-weight shortest paths from a list of source nodes on a static graph's source-major CSR (row_ptr [n+1] / col [m] int64, as
 * Graph.row_ptr / Graph.col hold them; n, m < 2^31, PP_ERR_TOO_LARGE from 2^31 on): what shortest_paths_dijkstra / diameter / avg_path_length,
 * src/pathpyG/algorithms/shortest_paths.py:13-52, get from scipy's Dijkstra with unweighted=True, and the distance totals behind
 * closeness_centrality, src/pathpyG/algorithms/centrality.py:327-356 (networkx: incoming distances).  One workgroup per source at a time,
 * level-synchronous frontier search; every stored edge counts once (parallel edges and self-loops are legal).  sources [n_sources] int64 node
 * indices in [0, n), repeats allowed (a source outside the range is skipped).  Every output may be NULL (reach_in and dist_in only together):
 *   dist [n_sources, n] int32: -1 = unreachable, 0 on the source itself;
 *   pred [n_sources, n] int32: predecessor on a shortest path, the LARGEST node index among the tight ones; -9999 (scipy) on the source
 *     itself and for unreachable nodes;
 *   reach_in [n] / dist_in [n] int64, ADDED to: number of sources s != v that reach v / sum of their distances;
 *   totals [3] int64, ADDED to (zero them first): sum of all finite distances to nodes other than the source, the largest finite distance,
 *     number of (source, node != source) pairs without a path.  Integer atomics only: independent of order.
 * ws: pp_graph_bfs_ws_bytes(n, n_sources), O(n) per workgroup, pp_graph_bfs_parts(n, n_sources) workgroups. */
int64_t pp_graph_bfs_parts(int64_t n, int64_t n_sources);
size_t pp_graph_bfs_ws_bytes(int64_t n, int64_t n_sources);
int pp_graph_bfs(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t m, const int64_t* sources, int64_t n_sources, int32_t* dist,
                 int32_t* pred, int64_t* reach_in, int64_t* dist_in, int64_t* totals, void* ws, size_t ws_bytes, pp_stream_t stream);

/* Betweenness centrality as the reference computes it (betweenness_centrality, src/pathpyG/algorithms/centrality.py:83-134: Brandes with
 * Python dicts per source), level-synchronous on the same CSR and source list (a repeated source counts twice, as in the loop of :105).
 * A source's contribution to node w is npred[w] * delta[w], npred the number of stored edges into w from the previous level: the
 * reference adds delta[w] once per entry of P[w] (:130-133).  partial [pp_graph_betweenness_parts(n, n_sources), n] float64: one row per
 * workgroup, the centrality of node v is the sum of column v over the rows (summed by the caller in row order: bit-reproducible; no
 * floating-point atomics in the dependencies).  reached [n] int32, zeroed by the caller, two bits per node: bit 0 is set for every node
 * that some source reached at distance >= 1 — the keys of the reference's result; bit 1 is set for every node to which some searched source
 * has 2^1024 or more shortest paths.  Path counts are float64 where the reference's are unbounded ints: exact (and the result
 * bit-reproducible) below 2^53, within summation rounding up to 2^1024, inf from there on — if any bit 1 is set, `partial` holds nothing of
 * use and the caller has to refuse the call.  ws: pp_graph_betweenness_ws_bytes(n, n_sources). */
int64_t pp_graph_betweenness_parts(int64_t n, int64_t n_sources);
size_t pp_graph_betweenness_ws_bytes(int64_t n, int64_t n_sources);
int pp_graph_betweenness(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t m, const int64_t* sources, int64_t n_sources,
                         double* partial, int32_t* reached, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ connected components (pp_graph_components.hip) */
/* Weakly or strongly connected components of a static graph: what connected_components / largest_connected_component,
 * src/pathpyG/algorithms/components.py:14-53, get from scipy.sparse.csgraph.connected_components on a host copy and from a Python loop over
 * graph.edges.  edge_index [2, m] int64 row-major (any order); n, m < 2^31, PP_ERR_TOO_LARGE from 2^31 on, before anything is launched.
 * Every stored edge counts; parallel edges and self-loops are legal and change nothing; an endpoint outside [0, n) is skipped, never
 * dereferenced.  n == 0 and m == 0 are legal.
 *   strong == 0: lock-free union-find over the edge list (path halving, atomicCAS hooking of the larger root under the smaller, after every
 *     node was hooked to its smallest smaller neighbour); the four CSR / CSC pointers are not read and may be NULL.
 *   strong != 0: forward colouring + backward search with trimming on the CSR (row_ptr [n+1], col [m]: out-edges) and the CSC (col_ptr [n+1],
 *     row [m]: in-edges) as Graph holds them; self-loops are ignored; edge_index is not read.  The number of sweeps grows with the longest
 *     shortest path (a directed ring of k nodes: about 2k launches).
 * labels [n] int32: components are numbered in the order of their SMALLEST node index (weak: scipy's numbering; strong: scipy's partition,
 * numbered this way instead of in Tarjan's completion order).  sizes [n] int64: the first *count entries are the component sizes, the rest
 * is zero.  count [1] int64.  labels, sizes and count are DEVICE pointers.  stats [4] is a HOST array or NULL: rounds, trim sweeps, colour
 * sweeps, backward sweeps (all 0 for strong == 0).  Integer atomics only: every output is the same on every run.
 * Fixpoints are host loops over launches with a device word read back in between (the call synchronises the stream when strong != 0); each is
 * bounded by n + 1 sweeps and the rounds by n: PP_ERR_HIP when a bound is hit.  ws: pp_graph_components_ws_bytes(n, m, strong). */
size_t pp_graph_components_ws_bytes(int64_t n, int64_t m, int strong);
int pp_graph_components(const int64_t* edge_index, int64_t m, int64_t n, const int64_t* row_ptr, const int64_t* col, const int64_t* col_ptr,
                        const int64_t* row, int strong, int32_t* labels, int64_t* sizes, int64_t* count, int64_t* stats, void* ws,
                        size_t ws_bytes, pp_stream_t stream);

/* out2 [2] int64 (device) = {label, size} of the largest of the first count[0] entries of sizes; among equal sizes the smallest label: the
 * choice of Counter(labels).most_common(1) under the numbering above (components.py:46-47).  {-1, 0} when count[0] == 0. */
int pp_graph_components_largest(const int64_t* sizes, const int64_t* count, int64_t* out2, pp_stream_t stream);

/* The sub-graph of one component, compacted in stored order with the scan of pp_scan.hip:
 * pp_graph_component_nodes: nodes_out [nodes_cap] int64 = the node indices v with labels[v] == keep, ascending (those beyond nodes_cap are
 *   not written); count_out [1] (device) their number.
 * pp_graph_component_edges: the stored edges whose two ends both carry the label `keep`, in stored order, renumbered through
 *   new_index [n] int64 (read only at kept nodes): edges_out [2, m] int64 with row stride m, the first count_out[0] columns of each row valid.
 * ws: pp_graph_component_keep_ws_bytes(n) / (m). */
size_t pp_graph_component_keep_ws_bytes(int64_t count);
int pp_graph_component_nodes(const int32_t* labels, int64_t n, int64_t keep, int64_t* nodes_out, int64_t nodes_cap, int64_t* count_out, void* ws,
                             size_t ws_bytes, pp_stream_t stream);
int pp_graph_component_edges(const int64_t* edge_index, int64_t m, int64_t n, const int32_t* labels, int64_t keep, const int64_t* new_index,
                             int64_t* edges_out, int64_t* count_out, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ order selection (pp_selection.hip) */

/* Index arrays below are int32 (`*_wide` = 0) or int64 (1): the level-by-level builders keep int32 CSR arrays, Graph.row_ptr is int64.
 * Status words (int64, 0 = fine): bit 0 an index outside its range (it was not read), bit 1 a row pointer array that is not ascending
 * from 0 to the entry count, bit 2 a node id in [0, n) that never occurs, bit 3 walk lengths that do not fit the store.
 *
 * pp_walk_counts_i64: the path counts of MultiOrderModel.get_mon_dof(assumption="paths"), src/pathpyG/core/multi_order_model.py:283-309,
 * without the k-1 line-graph lifts of :283-291 (lift_order_edge_index, lift_order.py:47-81) and without the sparse matrix power of
 * :293-309 — and the answer to the "TODO: can it be done together?" there: c_1[v] = out-degree(v), c_k[v] = sum of c_{k-1} over the
 * successors of v, pushed K times through the source-major CSR (row_ptr [n+1], col [n_edges]).
 *   out [3K + 1] int64: totals[k-1] = sum_v c_k[v] (walks of length k), starts[k-1] = #{v : c_k[v] > 0} (rows of the order-k transition
 *   matrix), saturated[k-1] = 1 when an addition of order k left int64 — every addition saturates at INT64_MAX, starts stay exact —
 *   and the status word.  Rows of more than 1024 entries are summed by a workgroup; the totals are integer sums (two 64-bit words, one atomic
 *   per workgroup and word): exact in any order.  ws: pp_walk_counts_ws_bytes(n, n_edges, K). */
size_t pp_walk_counts_ws_bytes(int64_t n, int64_t n_edges, int64_t K);
int pp_walk_counts_i64(const void* row_ptr, int ptr_wide, const void* col, int col_wide, int64_t n, int64_t n_edges, int64_t K, int64_t* out,
                       void* ws, size_t ws_bytes, pp_stream_t stream);

/* Two likelihood terms of one layer, from its source-major CSR (row_ptr [n_rows+1], weight [n_edges] float32), in float64:
 *   out2[0] = T = sum_e w_e log(w_e / S_row(e)), S the float64 sum of the row's weights: the top-order term of
 *     MultiOrderModel.get_mon_log_likelihood, multi_order_model.py:394-397 (Graph.transition_probabilities(edge_attr="edge_weight"),
 *     src/pathpyG/core/graph.py:518-533);
 *   out2[1] = I = sum_s freq_s log(1 / d(row of edge sel_s)), d the UNWEIGHTED out-degree: get_intermediate_order_log_likelihood,
 *     multi_order_model.py:338-369 (:363 calls transition_probabilities() without edge_attr), sel [n_sel] the layer's edge of the first
 *     transition of every surviving walk, freq [n_sel] float32 the walk weights; n_sel = 0: I = 0.  The row of an edge is found by
 *     binary search in row_ptr.
 * Both are pure functions of the input VALUES: fixed summation shapes (a row by 64 strided lanes, by 256 above 1024 entries; vectors
 * by chunks of 2048 whose partial sums one workgroup adds in index order), no floating-point atomics; zero and negative weights
 * follow IEEE arithmetic.  ws: pp_mon_layer_llh_ws_bytes(n_rows, n_edges, n_sel). */
size_t pp_mon_layer_llh_ws_bytes(int64_t n_rows, int64_t n_edges, int64_t n_sel);
int pp_mon_layer_llh_f64(const void* row_ptr, int ptr_wide, int64_t n_rows, const float* weight, int64_t n_edges, const void* sel, int sel_wide,
                         const float* freq, int64_t n_sel, double* out2, int64_t* status, void* ws, size_t ws_bytes, pp_stream_t stream);

/* The zeroth-order terms of a walk store (node_sequence [positions] int64, dag_num_nodes [walks] int64, dag_weight [walks] float32 as
 * PathData.append_walks leaves them, src/pathpyG/core/path_data.py:126-159; n = 1 + the largest node id), in float64:
 *   out2[0] = Z  = sum_w f_w log(c[first node of w] / positions), c the unweighted count of positions per node:
 *     get_zeroth_order_log_likelihood, multi_order_model.py:311-336;
 *   out2[1] = Z0 = sum_v C_v log(C_v / sum C), C_v the sum of the walk weights over the positions at v: the max_order = 0 branch of
 *     get_mon_log_likelihood, :402-407.  The positions are grouped by node with one stable radix sort, so C_v is added in position order.
 * Status bit 2 (an id of [0, n) without a position) or bit 0: the reference's torch.unique counts are then indexed by rank, not by id —
 * the caller keeps the torch route.  ws: pp_mon_zeroth_llh_ws_bytes(positions, walks, n). */
size_t pp_mon_zeroth_llh_ws_bytes(int64_t positions, int64_t walks, int64_t n);
int pp_mon_zeroth_llh_f64(const int64_t* node_sequence, int64_t positions, const int64_t* dag_num_nodes, const float* dag_weight, int64_t walks,
                          int64_t n, double* out2, int64_t* status, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ rolling time windows (pp_rolling.hip) */
/* The weighted static graph of EVERY window [start_w, end_w) of a time-sorted event stream (reference RollingTimeWindow,
 * src/pathpyG/algorithms/rolling_time_window.py:50-61: one TemporalGraph.to_static_graph(weighted=True, time_window=...) per window),
 * from one grouping of the stream.  edge_index [2, m] int64 row-major, time [m] int64 (time_dtype 1) or float64 (3), m < 2^31 - 16.
 *
 * pp_rolling_group: keys_out [m] = src << bits | dst of every event, ascending (bits = significant bits of num_nodes - 1; elements of
 *   pp_rolling_key_bytes(num_nodes) = 4 or 8 bytes), perm_out [m] the event (= time rank) at every position, stable: a node pair's events
 *   are one run of positions in time order.  flags [1]: bit 0 a node index outside [0, num_nodes), bit 1 the stream is not in timestamp
 *   order or holds a NaN.  With a flag set the other outputs are unspecified.  ws: pp_rolling_group_ws_bytes(m, num_nodes).
 * pp_rolling_bounds: lo[w] / hi[w] = first event with time >= starts[w] / >= ends[w] (m when there is none), starts / ends [W] in the dtype
 *   of `time`, W < 2^31 - 16.  Window w holds the events lo[w] <= e < hi[w].  starts and ends must be non-decreasing in w.
 * pp_rolling_count, for the windows w0 <= w < w1: cnt[j] = number of those windows in which position j is the first position of its pair
 *   whose event lies in the window.  report [w1 - w0 + 2] int32: report[k] - for k <= w1 - w0 - the difference array of the per-window
 *   edge counts (edges of window w0 + k = report[0] + ... + report[k]; the whole array sums to 0), report[w1 - w0 + 1] = flags[0], plus
 *   bit 2 when a pair has max_run events or more (max_run >= 1).
 * pp_rolling_fill, same windows, cnt as pp_rolling_count left it and total = the sum of cnt (< 2^31 - 16): the edges of the windows one
 *   window after the other, (src, dst)-sorted inside a window, to out_src / out_dst [total] int64 and out_weight [total] float32 (the
 *   number of the pair's events in the window); num_nodes_out [w1 - w0] uint32 = 1 + the largest node index of the window (2^31 for node
 *   2^31 - 1; num_nodes < 2^32), 0 for an empty one.  ws: pp_rolling_fill_ws_bytes(m, total). */
int pp_rolling_key_bytes(int64_t num_nodes);
size_t pp_rolling_group_ws_bytes(int64_t m, int64_t num_nodes);
int pp_rolling_group(const int64_t* edge_index, const void* time, int time_dtype, int64_t m, int64_t num_nodes, void* keys_out,
                     uint32_t* perm_out, int32_t* flags, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_rolling_bounds(const void* time, int time_dtype, int64_t m, const void* starts, const void* ends, int64_t W, int32_t* lo, int32_t* hi,
                      pp_stream_t stream);
int pp_rolling_count(const void* keys, int key_bytes, const uint32_t* perm, int64_t m, const int32_t* lo, const int32_t* hi, int64_t W,
                     int64_t w0, int64_t w1, int64_t max_run, const int32_t* flags, int32_t* cnt, int32_t* report, pp_stream_t stream);
size_t pp_rolling_fill_ws_bytes(int64_t m, int64_t total);
int pp_rolling_fill(const void* keys, int key_bytes, const uint32_t* perm, int64_t m, int64_t num_nodes, const int32_t* lo, const int32_t* hi,
                    int64_t W, int64_t w0, int64_t w1, const int32_t* cnt, int64_t total, int64_t* out_src, int64_t* out_dst, float* out_weight,
                    uint32_t* num_nodes_out, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ graph statistics (pp_graph_triads.hip) */
/* The sizes of the intersection of two sorted successor lists: what closed_triads / local_clustering_coefficient,
 * src/pathpyG/statistics/clustering.py:10-88, and the set-based measures of node_similarities.py:39-178 get from Python loops and sets.
 * All of them read the SIMPLE successor structure of a graph: row_ptr [n + 1] int64, col [ms] int64 strictly increasing inside a row,
 * row [ms] the row of every entry, mult [ms] int64 the number of stored parallel edges behind an entry (NULL: all 1).  A node index outside
 * [0, n) is never dereferenced (its list counts as empty); row pointers are clamped to [0, ms].  All pointers but ws contents are DEVICE
 * pointers; integer results are exact and every result is the same on every run.
 *
 * group: the number of lanes that share one pair of lists, a power of two up to 64; 0 = the smallest power of two no less than ms / n,
 *   between 4 and 64.  heavy_min: a pair whose SHORTER list has this many entries or more goes to a second launch with a workgroup per pair;
 *   0 = 1024.  Both change the time only, and the last bits of `aa`.
 *
 * pp_graph_count_unordered: out [1] = the number of positions e with (row, col)[e] >= (row, col)[e + 1] in edge_index [2, m] int64 row-major:
 *   0 means the stored list is (row, col)-sorted without parallel edges, i.e. it is its own simple structure.
 * pp_graph_triad_entry_counts: cnt [e1 - e0], cnt[e - e0] = |S(col[e]) n S(row[e])| for the entries e0 <= e < e1: the closed triads (x, y) of
 *   v = row[e] with x = col[e], self-loops included as the reference's sets include them.  ws: pp_graph_meet_ws_bytes(e1 - e0).
 * pp_graph_triad_node_counts: triads [n] = the sum of those counts over each row (a difference of their exclusive scan): the size of
 *   closed_triads(g, v) for every v.  ws: pp_graph_triad_node_counts_ws_bytes(ms).
 * pp_graph_pair_meets: for pairs [2, P] int64 row-major (v = pairs[p], w = pairs[P + p]): common[p] = |S(v) n S(w)|, dot[p] (or NULL) = the
 *   sum of mult_v(u) mult_w(u) over the common u, aa[p] (or NULL) = the sum of table[d(u)] over them, d(u) = deg_ptr[u + 1] - deg_ptr[u] the
 *   STORED out-degree (deg_ptr [n + 1] int64), table [table_len] float64 (d is clamped to table_len - 1).  The float64 sum has a fixed shape:
 *   the same bits on every call with the same structure, group and heavy_min, whatever else the batch holds.  sizes [2, P] (or NULL) = the
 *   lengths of the two lists.  ws: pp_graph_meet_ws_bytes(P).
 * pp_graph_triad_fill: the closed triads of the one node v as out [2, total] int64 row-major ((x, y) pairs, grouped by x in the order of
 *   v's row, y ascending); offset [offsets] = the exclusive scan of pp_graph_triad_entry_counts over v's row, total its sum. */
int pp_graph_count_unordered(const int64_t* edge_index, int64_t m, int64_t* out, pp_stream_t stream);
size_t pp_graph_meet_ws_bytes(int64_t tasks);
int pp_graph_triad_entry_counts(const int64_t* row_ptr, const int64_t* row, const int64_t* col, int64_t n, int64_t ms, int64_t e0, int64_t e1,
                                int group, int64_t heavy_min, int64_t* cnt, void* ws, size_t ws_bytes, pp_stream_t stream);
size_t pp_graph_triad_node_counts_ws_bytes(int64_t ms);
int pp_graph_triad_node_counts(const int64_t* row_ptr, const int64_t* row, const int64_t* col, int64_t n, int64_t ms, int group, int64_t heavy_min,
                               int64_t* triads, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_graph_pair_meets(const int64_t* row_ptr, const int64_t* col, const int64_t* mult, int64_t n, int64_t ms, const int64_t* pairs, int64_t P,
                        const int64_t* deg_ptr, const double* table, int64_t table_len, int group, int64_t heavy_min, int64_t* common,
                        int64_t* dot, double* aa, int64_t* sizes, void* ws, size_t ws_bytes, pp_stream_t stream);

/* out [P] float64 = one measure of node_similarities.py per pair, from the integers of pp_graph_pair_meets; NaN where the reference's scalar
 * function raises ZeroDivisionError.  Each value is an exact integer operation followed by correctly rounded float64 divisions / square roots:
 *   PP_PAIR_OVERLAP      common / min(sizes)               (NaN when a list is empty)            node_similarities.py:59-80
 *   PP_PAIR_JACCARD      common / (sizes - common), 1 when both lists are empty                 :83-113
 *   PP_PAIR_ADAMIC_ADAR  aa, 0 without a common neighbour                                       :116-145
 *   PP_PAIR_COSINE       dot / (sqrt(norm2[p]) sqrt(norm2[P + p])), norm2 [2, P] = the dot of each node with itself; 0 when the stored
 *                        in-degree indeg [n] (int32) of either node is 0, as the reference tests it       :148-178 */
enum { PP_PAIR_OVERLAP = 1, PP_PAIR_JACCARD = 2, PP_PAIR_ADAMIC_ADAR = 3, PP_PAIR_COSINE = 4 };
int pp_pair_measure(int measure, const int64_t* common, const int64_t* dot, const double* aa, const int64_t* sizes, const int64_t* norm2,
                    const int32_t* indeg, const int64_t* pairs, int64_t P, int64_t n, double* out, pp_stream_t stream);
int pp_graph_triad_fill(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t ms, int64_t v, const int64_t* offset, int64_t offsets,
                        int64_t total, int64_t* out, pp_stream_t stream);

/* out [1] int64 (device) = the sum over the stored edges of a[src] * b[dst] (a == NULL: of b[dst]), a, b [n] int32 degree vectors:
 * S_e of degree_assortativity, src/pathpyG/statistics/degrees.py:207-247, as an exact integer (int64 adds: the same in any order). */
int pp_degree_product_sum(const int64_t* edge_index, int64_t m, int64_t n, const int32_t* a, const int32_t* b, int64_t* out, pp_stream_t stream);

/* coeff [n] float64 (or NULL): triads[v] / (deg[v] (deg[v] - 1)), 0 where deg[v] <= 1 — one correctly rounded division of two exact
 * numbers, which is what local_clustering_coefficient, clustering.py:10-37, evaluates for either kind of graph (its undirected branch halves and
 * doubles the count).  mean [1] float64 (or NULL): the mean of the coefficients ROUNDED TO float32 (avg_clustering_coefficient, :67), summed
 * in float64 with a fixed shape and rounded to float32 at the end; NaN for n == 0.  ws: pp_graph_clustering_ws_bytes(). */
size_t pp_graph_clustering_ws_bytes(void);
int pp_graph_clustering(const int64_t* triads, const int32_t* deg, int64_t n, double* coeff, double* mean, void* ws, size_t ws_bytes,
                        pp_stream_t stream);

/* ------------------------------------------------------------------ colour refinement (pp_graph_wl.hip) */
/* Colour refinement (the 1-dimensional Weisfeiler-Leman iteration) of a static graph on its CSR (row_ptr [n + 1], col [m] int64, device):
 * the rounds of WeisfeilerLeman_test, src/pathpyG/algorithms/weisfeiler_leman.py:44-62, which build one Python string per node and round.
 * A node's signature is (own colour, multiset of the colours of its STORED successors): parallel edges count with their multiplicity, a
 * self-loop contributes the node's own colour, predecessors play no part.  n, m < 2^31 - 1, PP_ERR_TOO_LARGE from there on, before anything is
 * launched.  A column outside [0, n) is never dereferenced (it counts as one extra colour); row pointers are clamped to [0, m].
 *   initial [n] int64 (device) or NULL (all nodes equal): any values.  order [n] int64 (device) or NULL (index order): a permutation of
 *   0 .. n-1, the rank of every node; PP_ERR_ARG if it is none.  max_rounds < 0: refine until the class count stops growing.
 *   colours [n] int64 (device): the classes after the last round, numbered 0 .. k-1 by the first occurrence of a member in `order`.
 *   counts, passes [stats_cap] HOST arrays, rounds_out [1] HOST: counts[0] = the number of distinct initial colours, counts[r] the number of
 *   classes after round r = 1 .. *rounds_out; the last round of an unbounded call is the one that did not grow the count (its partition and
 *   numbers equal the previous round's).  passes[r] = the verify passes of round r (passes[0]: of the initial grouping, 0 without `initial`).
 *   n == 0: counts = {0} or, if a round was asked for, {0, 0}.  PP_ERR_ARG if stats_cap < rounds + 1 (n + 2 always suffices).
 *   seconds [3] HOST or NULL: when given, the stream is drained around every stage and the wall time is added up: [0] keys + sort,
 *   [1] the signature, election, verify and numbering kernels, [2] the grouping (unique rows).
 * Exactness: per round the m keys row * (k + 1) + colour[col] are sorted (pp_sort.hip), each node gets (own colour, degree, two 63-bit sums of
 * mixed colours AND hash_mask), nodes are grouped by these words (pp_unique_rows_count), and every node then compares its sorted row element by
 * element with that of the group's unresolved node of smallest rank (integer atomicMin); those that differ go through another election.  The
 * classes are exact for every hash_mask, 0 included; a weaker hash only adds verify passes.
 * group: the lanes that share one row, a power of two up to 64; 0 = the smallest power of two no less than m / n, between 4 and 64.
 * heavy_min: a row of this many entries or more gets a whole workgroup in a second launch; 0 = pp_graph_wl_heavy_min() = 1024.  Both change
 * the time only.  Integer work only: every output is the same on every run.  The round loop is a host loop over launches: the call
 * synchronises the stream once per verify pass (and once or twice before the first round).  ws: pp_graph_wl_ws_bytes(n, m). */
int64_t pp_graph_wl_heavy_min(void);
size_t pp_graph_wl_ws_bytes(int64_t n, int64_t m);
int pp_graph_wl_refine(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t m, const int64_t* initial, const int64_t* order,
                       int64_t max_rounds, int64_t hash_mask, int group, int64_t heavy_min, int64_t* colours, int64_t* counts, int64_t* passes,
                       int64_t stats_cap, int64_t* rounds_out, double* seconds, void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ random graph models (pp_random_graphs.hip)
 * Reference: src/pathpyG/algorithms/generative_models.py (G(n,p), G(n,m), stochastic block model, Watts-Strogatz), host loops there.
 * Every random word is one block of Philox4x32-10 keyed by the 64-bit `seed`; the counter is {index lo, index hi, stream lo,
 * tag << 24 | stream bits 32..55} and each use has its own tag below.  Integer arithmetic only; results do not depend on the grid (which
 * follows pp_set_launch_share).  uint64 quantities (seed, bound, threshold) travel as the int64 with the same bits.
 *   pp_rg_region_count / _fill: a Bernoulli subset of R regions of rank space, walked chunk by chunk with geometric skips.  regions
 *   [R, 8] int64 (device): {first chunk, slots N, log2 of the chunk's slots, skip constant c = -1 / log2(1 - p) with 32 fraction bits (< 2^63),
 *   kind, columns, row offset, column offset}; kind 0 rectangle (slot = row * columns + col), 1 strict lower triangle (slot = row (row - 1) / 2
 *   + col), 2 lower triangle with diagonal, 3 square without diagonal (columns = rows - 1, a column >= row is shifted by one).  First chunks
 *   ascend; a region without chunks shares its first chunk with the next one.  counts [n_chunks] int64; offsets [n_chunks + 1] its exclusive
 *   scan; rows, cols [total] int64: the edges in chunk order, ascending slots inside a chunk, offsets added; with perm ([n], rank -> node)
 *   both ends are mapped.  All ranks < n < 2^31 - 1.
 *   pp_rg_decode: slot -> (row, col) for `count` given slots of one region shape.
 *   pp_rg_draws: out[i] = the unbiased draw below `below` (uint64, != 0) with index first + i: multiply-high of a word, rejected while the low
 *   product word is under 2^64 mod below; attempt a of the draw reads stream `round << 32 | a`.
 *   pp_rg_first / _keep / _compact: the first m distinct values of a draw sequence, from its stable sort by value (value, draw index):
 *   first_by_draw[d] = 1 where draw d is the first occurrence of its value; with rank = the exclusive scan of that, keep[i] = sorted entry i is
 *   a first occurrence of rank < m; with pos = the exclusive scan of keep ([count + 1]), out[pos[i]] = value[i] for the kept (cap entries).
 *   pp_rg_complement: out[o], o < count: the o-th slot that is not in the ascending distinct list excluded[0 .. k).
 *   pp_rg_keys: keys[i] = rows[i] * n + cols[i].
 *   pp_rg_ws_edges: the ring lattice of n nodes and s neighbours, edge e = (k - 1) n + v being v -> (v + k) mod n, its column replaced by a
 *   uniform draw below n where the edge's decision word is under `threshold` (or `always`); undirected: the ends sorted.  rows, cols [n s].
 *   pp_rg_ws_offenders: from the stable sort (key, edge) of the keys: flag[edge] = 1 for every copy of a key but the one of smallest edge index
 *   (dups) and for every loop (loops).  pp_rg_ws_redraw: flagged edges get a new column drawn for (edge, round), the ends sorted if undirected. */
#define PP_RG_TAG_REGION 1
#define PP_RG_TAG_GNM 2
#define PP_RG_TAG_WS_DECIDE 3
#define PP_RG_TAG_WS_TARGET 4
#define PP_RG_TAG_WS_REPAIR 5
int pp_rg_region_count(const int64_t* regions, int64_t n_regions, int64_t n_chunks, int64_t seed, int64_t* counts, pp_stream_t stream);
int pp_rg_region_fill(const int64_t* regions, int64_t n_regions, int64_t n_chunks, int64_t seed, const int64_t* offsets, const int64_t* perm,
                      int64_t n, int64_t total, int64_t* rows, int64_t* cols, pp_stream_t stream);
int pp_rg_decode(const int64_t* slots, int64_t count, int kind, int64_t cols, int64_t* rows_out, int64_t* cols_out, pp_stream_t stream);
int pp_rg_draws(int64_t below, int64_t seed, int tag, int64_t round, int64_t first, int64_t count, int64_t* out, pp_stream_t stream);
int pp_rg_first(const int64_t* value, const int32_t* draw, int64_t count, int32_t* first_by_draw, pp_stream_t stream);
int pp_rg_keep(const int64_t* value, const int32_t* draw, const int64_t* rank, int64_t count, int64_t m, int32_t* keep, pp_stream_t stream);
int pp_rg_compact(const int64_t* value, const int64_t* pos, int64_t count, int64_t cap, int64_t* out, pp_stream_t stream);
int pp_rg_complement(const int64_t* excluded, int64_t k, int64_t count, int64_t* out, pp_stream_t stream);
int pp_rg_keys(const int64_t* rows, const int64_t* cols, int64_t count, int64_t n, int64_t* keys, pp_stream_t stream);
int pp_rg_ws_edges(int64_t n, int64_t s, int64_t seed, int64_t threshold, int always, int undirected, int64_t* rows, int64_t* cols,
                   pp_stream_t stream);
int pp_rg_ws_offenders(const int64_t* key, const int32_t* edge, int64_t count, int64_t n, int dups, int loops, int32_t* flag, pp_stream_t stream);
int pp_rg_ws_redraw(int64_t n, int64_t count, int64_t seed, int64_t round, int undirected, const int32_t* flag, int64_t* rows, int64_t* cols,
                    pp_stream_t stream);

/* Degree-sequence models (molloy_reed, k_regular_random, is_graphic_erdos_gallai of the reference's generative_models.py); DESIGN.md
 * "Degree-sequence models" has the rules.  S = the sum of the n degrees (S < 2^31 - 1, n < 2^31 - 1), M = S / 2 edges, stored as (min, max).
 *   pp_rg_mr_stubs: ptr [n + 1] the exclusive scan of the degrees (ptr[n] == stubs); node[s] = the node whose range of ptr holds stub s (int32,
 *   by bisection), key[s] = the word of (PP_RG_TAG_MR_SHUFFLE, stream 0, index s), all 64 bits (int64 with the uint64's bits).
 *   pp_rg_mr_pair: order [2 edges] = the stubs in the stable unsigned order of their keys; edge i joins node[order[2 i]] and node[order[2 i + 1]].
 *   pp_rg_mr_claim: claim [edges] uint32 is set to "none" (0xFFFFFFFF), then every flagged edge e draws its victim v_e below `edges` for
 *   (PP_RG_TAG_MR_VICTIM, round, e) and claim[v_e] = min(claim[v_e], e) (atomic; the result does not depend on the order).
 *   pp_rg_mr_swap (after pp_rg_mr_claim on the same stream, same arguments): a flagged e with v_e != e, claim[v_e] == e and claim[e] none
 *   proposes, with (a, b) = edge e and (c, d) = edge v_e — c and d exchanged when bit 0 of the word of (PP_RG_TAG_MR_SIDE, stream round << 32,
 *   e) is set — e' = (a, c), f' = (b, d), sorted.  bad(x) = x is a loop or (unless multi) x's key is in sorted_key [edges], the ascending keys
 *   row n + col the flags were made from.  Both edges are rewritten iff bad(e') + (bad(f') || (!multi && f' == e')) <= 1 + flag[v_e].
 *   pp_rg_eg_check: asc [n] the degrees in ASCENDING order, all in 0 .. n - 1, scan [n + 1] its exclusive scan, so that the descending
 *   sequence is d_i = asc[n - i] and its prefix sums are P_r = scan[n] - scan[n - r].  violated[0] (int32, zeroed by the call) becomes 1 when
 *   P_n is odd or P_r > r (r - 1) + r (c_r - r) + P_n - P_{c_r}, c_r = max(r, #{i : d_i > r}), for some r in 1 .. n. */
#define PP_RG_TAG_MR_SHUFFLE 6
#define PP_RG_TAG_MR_VICTIM 7
#define PP_RG_TAG_MR_SIDE 8
int pp_rg_mr_stubs(const int64_t* ptr, int64_t n, int64_t stubs, int64_t seed, int32_t* node, int64_t* key, pp_stream_t stream);
int pp_rg_mr_pair(const int32_t* node, const int32_t* order, int64_t edges, int64_t n, int64_t* rows, int64_t* cols, pp_stream_t stream);
int pp_rg_mr_claim(const int32_t* flag, int64_t edges, int64_t seed, int64_t round, uint32_t* claim, pp_stream_t stream);
int pp_rg_mr_swap(const int32_t* flag, const uint32_t* claim, const int64_t* sorted_key, int64_t edges, int64_t n, int64_t seed, int64_t round,
                  int multi, int64_t* rows, int64_t* cols, pp_stream_t stream);
int pp_rg_eg_check(const int64_t* asc, const int64_t* scan, int64_t n, int32_t* violated, pp_stream_t stream);

/* ------------------------------------------------------------------ power-iteration centralities (pp_graph_power.hip) */
/* eigenvector_centrality and katz_centrality as networkx 3.4 iterates them (the reference forwards both names to networkx on a DiGraph copy,
 * src/pathpyG/algorithms/centrality.py:327-356), on the PREDECESSOR lists of the distinct edges: col_ptr [n + 1], row [k] int64 (device),
 * weight [k] float64 or NULL (every entry 1).  n, k < 2^31 - 1.  A row index outside [0, n) is not dereferenced (it adds 0); pointers are
 * clamped to [0, k].  All values float64.
 *   PP_POWER_EIGENVECTOR: x0 = start / sum(start) (start == NULL: all ones); y[v] = x[v] + sum_u w(u, v) x[u]; norm = sqrt(sum y^2), 1 if that
 *     is 0; x' = y / norm; err = sum |x' - x|.  alpha, beta, beta_scalar and normalized are not read.
 *   PP_POWER_KATZ: x0 = start (NULL: zeros); x'[v] = alpha * (sum_u w(u, v) x[u]) + b[v], b = beta [n] or, if NULL, beta_scalar;
 *     err = sum |x' - x|.  values = x' * (1 / sqrt(sum x'^2)) if normalized and that norm is not 0, else x'.
 * The iteration stops at the FIRST iterate with err < threshold (false for a NaN err) or after max_iter >= 1 iterations.  values [n]
 * (device): that iterate, or the last one.  iterations, converged, grids [2] are HOST words: iterations done, the criterion held, and the
 * workgroups of the light and the heavy gather launch.
 * Launch scheme: one iteration is 2 to 4 plain launches (gather of the light rows, gather of the heavy rows if there are any, [eigenvector:
 * scale and error], decide): Katz 2, or 3 with heavy rows; eigenvector 3, or 4 with heavy rows.  No cooperative launch, no grid-wide barrier, no floating-point atomics.  The decision is taken on the device by
 * the one-workgroup decide kernel; every kernel reads the device's `done` word first and does nothing once it is set.  The host enqueues
 * `batch` iterations (0 = 16; otherwise >= 8; the last batch is cut to what max_iter leaves), synchronises the stream and reads {done,
 * iterations, buffer} once per batch.
 * Summation: a light row is summed by `group` lanes (a power of two up to 64; 0 = the smallest power of two no less than k / n, between 4
 * and 64), lane j adding entries j, j + group, ... in order, the lanes folded by a butterfly; a row of heavy_min entries or more (0 =
 * pp_graph_power_heavy_min() = 1024) by a whole workgroup in a second launch, thread j adding entries j, j + 256, ... .  sum y^2 and the
 * errors are per-workgroup partials of fixed shape, folded by workgroup index in a fixed shape.  Grids depend on n, group and the number of
 * heavy rows only: every output has the same bits on every run with the same graph and parameters.  ws: pp_graph_power_ws_bytes(n). */
enum { PP_POWER_EIGENVECTOR = 0, PP_POWER_KATZ = 1 };
int64_t pp_graph_power_heavy_min(void);
size_t pp_graph_power_ws_bytes(int64_t n);
int pp_graph_power_iterate(const int64_t* col_ptr, const int64_t* row, const double* weight, int64_t n, int64_t k, int mode, double alpha,
                           const double* beta, double beta_scalar, const double* start, int normalized, double threshold, int64_t max_iter,
                           int64_t batch, int group, int64_t heavy_min, double* values, int64_t* iterations, int64_t* converged, int64_t* grids,
                           void* ws, size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ node layouts (pp_graph_layout.hip) */
/* The layouts of the reference's visualisations/layout.py:69-269 that are arithmetic: Fruchterman-Reingold as networkx 3.4's dense routine
 * iterates it (the reference hands "spring" to networkx.spring_layout), random, circular, grid.  Positions are [n, 2] row-major on the
 * device, float64 except where stated.  n < 2^31 - 1, entries < 2^31 - 1, else PP_ERR_TOO_LARGE before any launch.
 *
 * Adjacency (what the reference gets from to_scipy_sparse_matrix -> from_scipy_sparse_array -> nx.Graph): symmetric, one entry per unordered
 * pair {u, v}, u != v, with a stored edge in either direction; its value is 1 (weight == NULL) or the weight [m] (float64) of the LAST such
 * edge in the stored order of edge_index [2, m] (int64).  Self-loops and edges with an end outside [0, n) give no entry.  CSR sorted by (row,
 * neighbour): ptr [n + 1], nbr [nnz] int64, w [nnz] float64.  pp_graph_layout_adj_count sorts the 2 m directed copies stably, flags the last
 * of every run and leaves nnz in the HOST word `nnz` (one synchronisation; needs 2 m < 2^31 - 1); pp_graph_layout_adj_fill, on the same
 * stream with the same workspace untouched in between, writes the three arrays.  ws: pp_graph_layout_adj_ws_bytes(m).
 *
 * pp_graph_layout_iterate: from pos (read, then overwritten with the result), at most `iterations` times
 *     disp_i = sum_j (p_i - p_j) (k^2 / max(d_ij, 0.01)^2 - A_ij max(d_ij, 0.01) / k);  len_i = |disp_i|, 0.1 where that is < 0.01;
 *     dp_i = disp_i (t / len_i), 0 where fixed[i] (uint8 [n] or NULL);  p_i += dp_i;  t -= dt;  stop if sqrt(sum |dp_i|^2) / n < threshold
 * (false for a NaN).  auto_t: t = 0.1 max(extent x, extent y) of pos and dt = t / (iterations + 1) are computed on the device, the
 * arguments t and dt are not read.  iterations_run, last_err (the last value of sqrt(sum |dp|^2) / n), grids [4] are HOST words; grids =
 * {target blocks, source chunks, workgroups of the light attraction launch, of the heavy one}.
 * Launch scheme: one iteration is 3 plain launches, 4 with heavy nodes (all-pairs repulsion; attraction over the CSR fused with the update;
 * [the same for heavy nodes]; decide).  No cooperative launch, no grid-wide barrier, no floating-point atomics.  Every kernel reads the
 * device's `done` word first and does nothing once it is set.  The host enqueues `batch` iterations (0 = 16), synchronises the stream and
 * reads the state words once per batch.
 * Summation: repulsion — a workgroup of `block` threads (0 = 256; 64, 128, 256) owns `block` targets and one of `chunks` equal pieces of the
 * source range (0 = enough for about 2048 workgroups, at most 64 and at most n / 256 rounded up: pp_graph_layout_chunks); a thread adds the
 * sources of its piece in order into four accumulators (source j of the piece: accumulator j mod 4), folded (0 + 1) + (2 + 3); the pieces of
 * a node are added in order.  Attraction — `group` lanes per node (a power of two up to 64; 0 = the smallest power of two no less than
 * nnz / n, between 4 and 64), lane j adding entries j, j + group, ..., folded by a butterfly; a node of heavy_min entries or more (0 =
 * pp_graph_layout_heavy_min() = 1024) by a whole workgroup, thread j adding entries j, j + 256, ... .  sum |dp|^2: per-workgroup partials
 * folded by index in a fixed shape.  Every output has the same bits on every run with the same inputs and settings; `batch` never changes a
 * bit.  ws: pp_graph_layout_ws_bytes(n, block, chunks).
 *
 * pp_graph_layout_rescale: networkx.rescale_layout, then + center: p -= mean per axis; p *= scale / max |p| if that is > 0; p += (cx, cy).
 * pp_graph_layout_start: pos[v] = given[v] where given != NULL and (has == NULL or has[v], uint8), else uniform[0, 1) * dom_size + center,
 * the uniform being the top 53 bits of the Philox word of (seed, PP_RG_TAG_LAYOUT, stream 0, index 2 v + axis) times 2^-53.
 * pp_graph_layout_random: float32 [n, 2]: the top 24 bits of the same words times 2^-24, + center in float32.
 * pp_graph_layout_closed_form: PP_LAYOUT_CIRCULAR: (cos, sin) in float32 of the float32 angle 2 pi v / n, widened; PP_LAYOUT_GRID: with
 * s = floor(sqrt(n)): (v mod s, -floor(v / s)) / s. */
#define PP_RG_TAG_LAYOUT 9
enum { PP_LAYOUT_CIRCULAR = 0, PP_LAYOUT_GRID = 1 };
int64_t pp_graph_layout_heavy_min(void);
int64_t pp_graph_layout_chunks(int64_t n, int block, int64_t chunks);
size_t pp_graph_layout_ws_bytes(int64_t n, int block, int64_t chunks);
int pp_graph_layout_iterate(const int64_t* ptr, const int64_t* nbr, const double* w, int64_t n, int64_t nnz, double* pos, const uint8_t* fixed,
                            double k, double t, double dt, int auto_t, int64_t iterations, double threshold, int64_t batch, int block,
                            int64_t chunks, int group, int64_t heavy_min, int64_t* iterations_run, double* last_err, int64_t* grids, void* ws,
                            size_t ws_bytes, pp_stream_t stream);
size_t pp_graph_layout_rescale_ws_bytes(void);
int pp_graph_layout_rescale(double* pos, int64_t n, double scale, double cx, double cy, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_graph_layout_start(int64_t seed, int64_t n, double dom_size, double cx, double cy, const double* given, const uint8_t* has, double* pos,
                          pp_stream_t stream);
int pp_graph_layout_random(int64_t seed, int64_t n, float cx, float cy, float* pos, pp_stream_t stream);
int pp_graph_layout_closed_form(int kind, int64_t n, double* pos, pp_stream_t stream);
size_t pp_graph_layout_adj_ws_bytes(int64_t m);
int pp_graph_layout_adj_count(const int64_t* edge_index, int64_t m, int64_t n, int64_t* nnz, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_graph_layout_adj_fill(const double* weight, int64_t m, int64_t n, int64_t nnz, int64_t* ptr, int64_t* nbr, double* w, void* ws,
                             size_t ws_bytes, pp_stream_t stream);

/* ------------------------------------------------------------------ random walks (pp_walks.hip) */
/* Walks on a row-sorted CSR (row_ptr [n + 1], col [m] int64, device): a Graph, or a layer of a MultiOrderModel (no counterpart in the reference
 * snapshot; upstream pathpyG samples in Python loops).  Every output is a pure function of (seed, graph, weights, arguments): the words are
 * the Philox words of the random graph models above, under the tags below; the grid follows pp_set_launch_share and changes no bit.  No
 * floating-point atomics.  A uniform is x(word) = (double)(word >> 11) * 2^-53.  All arithmetic is float64 and every operation named below
 * is ONE rounded operation (nothing is contracted).  Pointers are clamped as everywhere (into [0, m], never descending).
 * Sizes: n, m, walks, steps, order < 2^31 - 1 and walks * (steps + order) < 2^31 - 1, else PP_ERR_TOO_LARGE before any launch;
 * pp_walk_check_sizes is that test alone (host code).
 *
 * pp_walk_table: weight [m] float32 or float64 (weight_dtype PP_F32 / PP_F64) widened to float64, NULL = all ones.  cum [m]: cum[j] = the
 *   left-to-right running sum of the weights of j's row from the row's first entry to j (row-local: s = 0; s = s + w; one lane per row).
 *   total [n]: T_v = the cum of v's last entry, 0 for an empty row.  bad [1] int32 (zeroed by the call) becomes 1 if a weight is negative,
 *   NaN or infinite, or a T_v is infinite.
 * pp_walk_start_table (start "weighted"): nodes in blocks of 1024 (pp_walk_start_blocks(n) of them).  bcum [n]: the left-to-right running sum
 *   of T_v inside the node's block (one lane per block); block_cum [blocks] = B: the left-to-right running sum of the blocks' totals (the
 *   bcum of each block's last node), by one lane.
 * pp_walk_positive_flag / _list (start "uniform"): flag[v] = T_v > 0 (int32); with pos [n + 1] the exclusive scan of the flags and count =
 *   pos[n], list [count] int32 = those nodes ascending.
 * pp_walk_run: one lane per walk w, the step loop inside the kernel.  The start node is
 *     start_mode 0: start_nodes[w] (int64; outside [0, n): the walk has no node, nodes[0][w] = -1, length 0);
 *     start_mode 1: target = x(word(seed, PP_RG_TAG_WALK_START, stream 0, index w)) * B[last]; b = the first block with B[b] > target (the last
 *       block if there is none); t2 = target - (b ? B[b - 1] : 0); the first node of block b with bcum > t2; if there is none (rounding), the
 *       block's last node with T_v > 0;
 *     start_mode 2: positive[d], d = the unbiased draw below positive_count by pp_rg_draws' rule (multiply-high, rejected while the low
 *       product word is under 2^64 mod positive_count; attempt a reads the word of (PP_RG_TAG_WALK_START, stream a, index w)).
 *   At step t = 0 .. steps - 1, at node v with entries [lo, hi): if the row is empty or not T_v > 0 the walk ends with length t (edges).
 *   Otherwise target = x(word(seed, PP_RG_TAG_WALK_STEP, stream t, index w)) * T_v, j = the smallest index of [lo, hi) with cum[j] > target
 *   (bisection bounded to the row) and the next node is col[j]; a column outside [0, n) ends the walk.  An entry of weight 0 is never chosen
 *   (its cum equals its predecessor's, or is 0 at the row's start, and target >= 0).  target < T_v ALWAYS holds for a finite positive normal
 *   T_v (x <= 1 - 2^-53, and x * T rounds below T), so the bound hi is never the answer; for a subnormal T_v where it could be, the walk ends.
 *   nodes [steps + 1, walks] int32, STEP-MAJOR (a wave's stores at one step are contiguous), -1 after a walk's end; lengths [walks] int32.
 *   `order` only enters the size test.
 * pp_walk_pack_count / _fill: the walk store of PathData from the step-major buffer.  keep[w] = length > 0, count[w] = order + length where
 *   kept, else 0 (int32).  With offset / rank [walks + 1] the exclusive scans of count / keep, positions = offset[walks], kept = rank[walks]
 *   and node_sequence [n, order] int64 the graph's: seq_out [positions] int64 = per kept walk the `order` first-order nodes of its first
 *   node, then the LAST first-order node of every later one; edge_src / edge_dst [positions - kept]: the chain p -> p + 1 inside every walk;
 *   dag_num_nodes / dag_num_edges [kept] int64 = order + length, that minus one; dag_weight [kept] float32 = 1.  Walks without an edge are
 *   left out. */
#define PP_RG_TAG_WALK_START 10
#define PP_RG_TAG_WALK_STEP 11
int pp_walk_check_sizes(int64_t n, int64_t m, int64_t walks, int64_t steps, int64_t order);
int pp_walk_table(const int64_t* row_ptr, int64_t n, int64_t m, const void* weight, int weight_dtype, double* cum, double* total, int32_t* bad,
                  pp_stream_t stream);
int64_t pp_walk_start_blocks(int64_t n);
int pp_walk_start_table(const double* total, int64_t n, double* bcum, double* block_cum, pp_stream_t stream);
int pp_walk_positive_flag(const double* total, int64_t n, int32_t* flag, pp_stream_t stream);
int pp_walk_positive_list(const int64_t* pos, int64_t n, int64_t count, int32_t* list, pp_stream_t stream);
int pp_walk_run(const int64_t* row_ptr, const int64_t* col, const double* cum, const double* total, int64_t n, int64_t m, int64_t walks, int64_t steps,
                int64_t order, int64_t seed, int start_mode, const int64_t* start_nodes, const double* bcum, const double* block_cum,
                const int32_t* positive, int64_t positive_count, int32_t* nodes, int32_t* lengths, pp_stream_t stream);
int pp_walk_pack_count(const int32_t* lengths, int64_t walks, int64_t steps, int64_t order, int32_t* keep, int32_t* count, pp_stream_t stream);
int pp_walk_pack_fill(const int32_t* nodes, const int32_t* lengths, int64_t walks, int64_t steps, int64_t order, int64_t n,
                      const int64_t* node_sequence, const int64_t* offset, const int64_t* rank, int64_t positions, int64_t kept,
                      int64_t* seq_out, int64_t* edge_src, int64_t* edge_dst, int64_t* dag_num_nodes, int64_t* dag_num_edges, float* dag_weight,
                      pp_stream_t stream);

/* ------------------------------------------------------------------ distributions and PageRank (pp_graph_diffusion.hip) */
/* The deterministic half of a random-walk process: B distributions at once, pushed through the transition structure of a Graph or of a layer
 * of a MultiOrderModel.  The structure is the MERGED one: row_ptr [n + 1] of Graph.simple_successors() and, for the pull, col_ptr [n + 1],
 * src [k] int64 and perm [k] int64 of Graph.simple_predecessors() (perm[j] = the successor position of pull entry j).  weight [k] float64 in
 * SUCCESSOR order, NULL = every entry 1.  A block X is [n, B] float64 row-major, B a power of two up to 64 (the padded width; `live` of the
 * columns count, the others stay as they are); a wider batch runs in column tiles of 64 from the host, which by (b) changes nothing.
 * All arithmetic is float64 and every operation named below is ONE rounded operation (nothing is contracted).  Pointers are clamped as
 * everywhere; a source index outside [0, n) adds 0.
 * Sizes: n, k < 2^31 - 1 and n * B * 8 * (kept blocks) < 2^47 bytes, else PP_ERR_TOO_LARGE before any launch; pp_diffusion_check_sizes is
 * that test alone (host code).
 *
 * pp_diffusion_table: T_u = the left-to-right sum of u's merged entries (s = 0; s = s + w; one lane per row) -> total [n];
 *   prob[j] = w / T_u for pull entry j of source u, 0 where T_u is 0 -> prob [k]; dangling[u] = !(T_u > 0) -> uint8 [n].  bad [1] int32
 *   (zeroed by the call) becomes 1 for a negative, NaN or infinite weight or an infinite T_u.
 * pp_diffusion_run: with s[v] = sum_i prob_i * x[src_i] over v's pull list and D = sum of x[u] over the dangling u, one iteration is
 *     PP_DIFFUSION_PAGERANK: x'[v] = alpha * (s[v] + D * d[v]) + (1 - alpha) * p[v]        (p, d [n, B]; networkx 3.4's order)
 *     PP_DIFFUSION_WALK    : x'[v] = lazy * x[v] + (1 - lazy) * (s[v] + (dangling[v] ? x[v] : 0))
 *   and err_c = sum |x' - x| per column c.  X [kept, n, B]: X[0] holds the start.  kept == 2: the iterates alternate between the two blocks;
 *   kept == max_iter + 1: iterate t is left in X[t].  A column stops at its FIRST iterate with err_c < threshold (false for a NaN; a negative
 *   threshold never holds: exactly max_iter iterations) and keeps exactly that iterate whatever the others still do; the run ends when all
 *   live columns have stopped, or after max_iter >= 0 iterations.  iterations [B], converged [B], where [1], grids [2] are HOST words: per
 *   column the iterations done and whether the criterion held, the block of X that holds the result, the workgroups of the row and of the
 *   heavy launch.  tvd (device, [max_iter + 1, B], or NULL; needs target [n]): tvd[t, c] = 0.5 * sum |x_t - target|, t = 0 .. max_iter
 *   (meant for a negative threshold; a stopped column's later rows are not written).
 *   Launch scheme: per iteration 2 plain launches, 3 with heavy rows (heavy rows; all rows, update and partials; decide, one workgroup per
 *   column).  No cooperative launch, no grid-wide barrier, no floating-point atomics (the decide kernel counts its arrived workgroups with
 *   one integer atomic).  Every kernel reads the run's `done` word first and does nothing once it is set.  The host enqueues `batch`
 *   iterations (0 = 16; the last batch is cut to what max_iter leaves), synchronises and reads the state words once per batch.
 *   Summation — the shapes are functions of a row's length, of n and of heavy_min only:
 *     a row of fewer than heavy_min entries (0 = pp_diffusion_heavy_min() = 1024): entry i of the row into accumulator i mod 4, in order; the
 *       sum is (a0 + a1) + (a2 + a3).  A row of heavy_min entries or more: chunks of 256 entries, each summed that way, added in order to 0.0;
 *     D, err, tvd: per range of 256 nodes, each group of 4 consecutive nodes is summed ((t0 + t1) + t2) + t3, the groups are added in order to
 *       0.0; the ranges are folded by index: thread t of 256 adds ranges t, t + 256, ... in order, then a wave butterfly, the 4 waves in order.
 *   Properties:
 *     (a) every output has the same bits on every run;
 *     (b) the bits of a column do not depend on B, on which columns share its block, or on their values: a lane pair (row, column) does
 *         the same operations in the same order whatever B is, the partials are per (range, column) and every column is folded and decided
 *         by a workgroup of its own.  A batch equals its columns run one by one;
 *     (c) pp_set_launch_share and `batch` change no bit (the grid strides over ranges whose partials do not depend on it);
 *     (d) max_iter is honoured exactly, also when it is no multiple of the batch.
 *   ws: pp_diffusion_ws_bytes(n, B).
 * pp_diffusion_project: out[r, c] = sum of x[idx[i], c] over i in [ptr[r], ptr[r + 1]) (ptr [rows + 1], idx [k] int64 into the n_src rows of
 *   x [n_src, B]), in the row shapes above: the first-order projection of a layer, with the layer nodes grouped by their last first-order
 *   node and ascending inside a group.  out [rows, B].  ws: pp_diffusion_ws_bytes(rows, B). */
enum { PP_DIFFUSION_PAGERANK = 0, PP_DIFFUSION_WALK = 1 };
int64_t pp_diffusion_heavy_min(void);
int pp_diffusion_check_sizes(int64_t n, int64_t k, int64_t B, int64_t kept);
int pp_diffusion_table(const int64_t* row_ptr, const double* weight, const int64_t* src, const int64_t* perm, int64_t n, int64_t k, double* total,
                       double* prob, uint8_t* dangling, int32_t* bad, pp_stream_t stream);
size_t pp_diffusion_ws_bytes(int64_t rows, int64_t B);
int pp_diffusion_run(const int64_t* col_ptr, const int64_t* src, const double* prob, const uint8_t* dangling, int64_t n, int64_t k, int B, int live,
                     int mode, double alpha, double lazy, const double* p, const double* d, const double* target, double* X, int64_t kept,
                     double threshold, int64_t max_iter, int64_t batch, int64_t heavy_min, int64_t* iterations, int64_t* converged, int64_t* where,
                     double* tvd, int64_t* grids, void* ws, size_t ws_bytes, pp_stream_t stream);
int pp_diffusion_project(const int64_t* ptr, const int64_t* idx, int64_t rows, int64_t n_src, int64_t k, const double* x, int B, double* out,
                         int64_t heavy_min, void* ws, size_t ws_bytes, pp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PATHPYG_AMD_H */
