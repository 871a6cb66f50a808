// pathpyg_amd — unit-weight shortest paths and betweenness on a static Graph's CSR.
//
// Reference: shortest_paths_dijkstra / diameter / avg_path_length, src/pathpyG/algorithms/shortest_paths.py:13-52 (scipy's Dijkstra with
// unweighted=True on the adjacency matrix: a dense n x n result per call), betweenness_centrality, src/pathpyG/algorithms/centrality.py:83-134
// (Brandes as pure-Python dict / list loops per source) and closeness_centrality, centrality.py:327-356 (networkx on a Python copy).
// With unit weights all of them are breadth-first searches from independent sources.  Here one workgroup takes the sources
// blockIdx.x, blockIdx.x + gridDim.x, ... and runs a level-synchronous frontier search on the source-major CSR (row_ptr [n+1], col [m],
// as Graph.row_ptr / Graph.col hold them).  All per-source state is per NODE (level, one order array, and for Brandes sigma, dep, npred,
// level starts) and lives in the workgroup's slice of a caller-provided workspace: O(n) bytes per workgroup, nothing per edge.
// Every stored edge counts once: parallel edges double a path count, self-loops are never tight — the kernels need no special case.
//
// Frontier expansion: a wave takes 64 consecutive frontier entries, one lane each.  Lanes whose node has fewer than 64 out-edges walk
// them alone; every node with 64 or more (hubs of an aggregated scale-free stream) is then expanded by the whole wave, lanes across its
// neighbours, so a hub row never serialises on one lane.
#include "pp_common.h"
#include "pp_internal.h"

namespace pp {

constexpr int32_t kNoPred = -9999;                   // scipy's "no predecessor"

// visit(v, payload(v), w) for every stored edge (v, w) of the frontier order[begin, end).  `payload` is read once per frontier node.
template <typename Payload, typename Visit>
__device__ __forceinline__ void expand_frontier(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col, const int32_t* order,
                                                int begin, int end, Payload&& payload, Visit&& visit) {
    for (int64_t base = (int64_t)begin + wave_id() * kWave; base < end; base += kBlock) {   // (wave-uniform trip count: the shuffles below; 64 bits: end may be 2^31 - 1)
        const int64_t k = base + lane_id();
        int32_t v = -1, p0 = 0, p1 = 0;                                                 // m < 2^31: edge positions fit 32 bits (strided ones are stepped in 64)
        double x = 0.0;
        if (k < end) {
            v = order[k];
            p0 = (int32_t)row_ptr[v];
            p1 = (int32_t)row_ptr[v + 1];
            x = payload(v);
        }
        const bool hub = p1 - p0 >= kWave;
        if (!hub)
            for (int32_t p = p0; p < p1; ++p) visit(v, x, col[p]);
        unsigned long long hubs = __ballot(hub);
        while (hubs) {
            const int owner = __ffsll((long long)hubs) - 1;
            hubs &= hubs - 1;
            const int32_t hv = __shfl(v, owner, kWave), h0 = __shfl(p0, owner, kWave), h1 = __shfl(p1, owner, kWave);
            const double hx = __shfl(x, owner, kWave);
            for (int64_t p = (int64_t)h0 + lane_id(); p < h1; p += kWave) visit(hv, hx, col[p]);
        }
    }
}

// dist / pred / reach_in+dist_in / totals: each may be null.  ws: 2 * max(n, 1) int32 per workgroup (level, order).
__global__ __launch_bounds__(kBlock) void k_graph_bfs(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col, int64_t n,
                                                     const int64_t* __restrict__ sources, int64_t n_sources, int32_t* __restrict__ dist,
                                                     int32_t* __restrict__ pred, int64_t* __restrict__ reach_in, int64_t* __restrict__ dist_in,
                                                     int64_t* __restrict__ totals, int32_t* __restrict__ ws) {
    __shared__ int s_tail;
    int32_t* level = ws + (size_t)blockIdx.x * 2 * (size_t)n;
    int32_t* order = level + n;
    for (int64_t v = threadIdx.x; v < n; v += kBlock) level[v] = -1;
    long long sum_dist = 0, max_dist = 0, no_path = 0;                                  // thread 0 keeps the workgroup's scalars
    __syncthreads();
    for (int64_t i = blockIdx.x; i < n_sources; i += gridDim.x) {
        const int64_t s = sources[i];
        if (s < 0 || s >= n) continue;                                                  // (the callers validate; nothing is written for such a source)
        int32_t* prow = pred ? pred + i * n : nullptr;
        if (prow)
            for (int64_t v = threadIdx.x; v < n; v += kBlock) prow[v] = kNoPred;
        if (threadIdx.x == 0) { level[s] = 0; order[0] = (int32_t)s; s_tail = 1; }
        __syncthreads();
        int begin = 0, depth = 0;
        while (true) {
            const int end = s_tail;
            __syncthreads();                                                            // everybody has read the tail before anybody appends
            if (begin == end) break;
            if (threadIdx.x == 0 && depth > 0) { sum_dist += (long long)depth * (end - begin); max_dist = max(max_dist, (long long)depth); }
            expand_frontier(row_ptr, col, order, begin, end, [](int32_t) { return 0.0; }, [&](int32_t v, double, int64_t w) {
                if ((uint64_t)w >= (uint64_t)n) return;
                const int32_t old = atomicCAS(&level[w], -1, depth + 1);
                if (old == -1) order[atomicAdd(&s_tail, 1)] = (int32_t)w;               // claimed once: the tail never passes n
                if (prow && (old == -1 || old == depth + 1)) atomicMax(&prow[w], v);    // tight edge: the largest predecessor index wins
            });
            __syncthreads();
            begin = end;
            ++depth;
        }
        const int tail = begin;
        if (threadIdx.x == 0) no_path += n - tail;
        if (dist) {
            int32_t* drow = dist + i * n;
            for (int64_t v = threadIdx.x; v < n; v += kBlock) drow[v] = level[v];
            __syncthreads();
        }
        for (int64_t k = threadIdx.x; k < tail; k += kBlock) {                              // per-node totals; the slice is clean for the next source
            const int32_t v = order[k];
            if (k > 0 && reach_in) {
                atomicAdd((unsigned long long*)&reach_in[v], 1ull);
                atomicAdd((unsigned long long*)&dist_in[v], (unsigned long long)level[v]);
            }
            level[v] = -1;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && totals) {
        atomicAdd((unsigned long long*)&totals[0], (unsigned long long)sum_dist);
        atomicMax((unsigned long long*)&totals[1], (unsigned long long)max_dist);
        atomicAdd((unsigned long long*)&totals[2], (unsigned long long)no_path);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Brandes' betweenness in the reference's own form (centrality.py:83-134), level-synchronous:
//   forward : BFS levels; sigma[w] += sigma[v] and npred[w] += 1 for every stored edge (v, w) from the previous level (centrality.py:119-126;
//             integer-valued doubles: below 2^53 the atomic adds are exact in any order and the result has the same bits on every run;
//             from 2^53 to 2^1024 they round, in an order that may differ from run to run, and the result is within summation rounding of
//             the reference's unbounded ints; a count of 2^1024 or more is inf and cannot be matched in float64 at all (inf / inf, x / inf):
//             the search ORs 2 into reached[v] of such a node v and the caller refuses the call — per searched source, not per graph);
//   backward: deepest level first; dep[v] = sum over v's out-edges to the next level of sigma[v] / sigma[w] * (1 + dep[w]) in CSR order
//             (a hub: lane j sums the entries j, j + 64, ... and the 64 partial sums meet in a fixed butterfly) — no floating-point atomics;
//   credit  : bw[w] += npred[w] * dep[w]: the reference adds delta[w] to bw[w] INSIDE its loop over P[w] (centrality.py:130-133), once per
//             predecessor edge, not once per node.  The source has no predecessor and gets nothing.
struct GraphBwWs {
    int32_t* level;
    int32_t* order;
    int32_t* npred;
    int32_t* level_start;
    double* sigma;
    double* dep;
};

__host__ __device__ static inline size_t graph_bw_block_bytes(int64_t n) {
    const size_t ne = (size_t)(n > 0 ? n : 1);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    return 3 * up(ne * 4) + up((ne + 2) * 4) + 2 * up(ne * 8);
}

__device__ static inline GraphBwWs carve_graph_bw(char* base, int64_t n) {
    const size_t ne = (size_t)(n > 0 ? n : 1);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    GraphBwWs w;
    w.level = (int32_t*)base; base += up(ne * 4);
    w.order = (int32_t*)base; base += up(ne * 4);
    w.npred = (int32_t*)base; base += up(ne * 4);
    w.level_start = (int32_t*)base; base += up((ne + 2) * 4);
    w.sigma = (double*)base; base += up(ne * 8);
    w.dep = (double*)base;
    return w;
}

__global__ __launch_bounds__(kBlock) void k_graph_betweenness(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col, int64_t n,
                                                             const int64_t* __restrict__ sources, int64_t n_sources,
                                                             double* __restrict__ bw_blocks, int32_t* __restrict__ reached, char* __restrict__ ws,
                                                             size_t block_bytes) {
    __shared__ int s_tail;
    const GraphBwWs w = carve_graph_bw(ws + (size_t)blockIdx.x * block_bytes, n);
    double* bw = bw_blocks + (int64_t)blockIdx.x * n;
    for (int64_t v = threadIdx.x; v < n; v += kBlock) { bw[v] = 0.0; w.level[v] = -1; w.npred[v] = 0; w.sigma[v] = 0.0; }
    __syncthreads();
    for (int64_t i = blockIdx.x; i < n_sources; i += gridDim.x) {
        const int64_t s = sources[i];
        if (s < 0 || s >= n) continue;
        if (threadIdx.x == 0) { w.level[s] = 0; w.order[0] = (int32_t)s; w.sigma[s] = 1.0; w.level_start[0] = 0; s_tail = 1; }
        __syncthreads();
        int begin = 0, depth = 0;
        while (true) {
            const int end = s_tail;
            __syncthreads();
            if (begin == end) break;
            if (threadIdx.x == 0) w.level_start[depth + 1] = end;
            auto count_of = [&](int32_t v) {                                             // every reached node is a frontier entry exactly once
                const double sv = w.sigma[v];
                if (sv > __DBL_MAX__) atomicOr(&reached[v], 2);                          // 2^1024 or more shortest paths: the caller refuses
                return sv;
            };
            expand_frontier(row_ptr, col, w.order, begin, end, count_of, [&](int32_t, double sv, int64_t x) {
                if ((uint64_t)x >= (uint64_t)n) return;
                const int32_t old = atomicCAS(&w.level[x], -1, depth + 1);
                if (old == -1) w.order[atomicAdd(&s_tail, 1)] = (int32_t)x;
                if (old == -1 || old == depth + 1) { atomicAdd(&w.sigma[x], sv); atomicAdd(&w.npred[x], 1); }
            });
            __syncthreads();
            begin = end;
            ++depth;
        }
        const int tail = begin;                                                          // levels 0 .. depth - 1 are order[level_start[d], level_start[d + 1])
        for (int d = depth - 1; d >= 1; --d) {
            const int lo = w.level_start[d], hi = w.level_start[d + 1];
            auto term = [&](double sv, int64_t x) {
                if ((uint64_t)x >= (uint64_t)n || w.level[x] != d + 1) return 0.0;
                return sv / w.sigma[x] * (1.0 + w.dep[x]);
            };
            auto finish = [&](int32_t v, double acc) {
                w.dep[v] = acc;
                bw[v] += (double)w.npred[v] * acc;
                if (!(reached[v] & 1)) atomicOr(&reached[v], 1);                         // (an OR: bit 1 of another search's refusal survives)
            };
            for (int64_t base = (int64_t)lo + wave_id() * kWave; base < hi; base += kBlock) {
                const int64_t k = base + lane_id();
                int32_t v = -1, p0 = 0, p1 = 0;
                double sv = 0.0;
                if (k < hi) {
                    v = w.order[k];
                    p0 = (int32_t)row_ptr[v];
                    p1 = (int32_t)row_ptr[v + 1];
                    sv = w.sigma[v];
                }
                const bool hub = p1 - p0 >= kWave;
                if (k < hi && !hub) {
                    double acc = 0.0;
                    for (int32_t p = p0; p < p1; ++p) acc += term(sv, col[p]);
                    finish(v, acc);
                }
                unsigned long long hubs = __ballot(hub);
                while (hubs) {
                    const int owner = __ffsll((long long)hubs) - 1;
                    hubs &= hubs - 1;
                    const int32_t hv = __shfl(v, owner, kWave), h0 = __shfl(p0, owner, kWave), h1 = __shfl(p1, owner, kWave);
                    const double hsv = __shfl(sv, owner, kWave);
                    double part = 0.0;
                    for (int64_t p = (int64_t)h0 + lane_id(); p < h1; p += kWave) part += term(hsv, col[p]);
                    part = wave_sum(part);
                    if (lane_id() == 0) finish(hv, part);
                }
            }
            __syncthreads();
        }
        for (int64_t k = threadIdx.x; k < tail; k += kBlock) {                              // the slice is clean for the next source
            const int32_t v = w.order[k];
            w.level[v] = -1;
            w.npred[v] = 0;
            w.sigma[v] = 0.0;
        }
        __syncthreads();
    }
}

}  // namespace pp

extern "C" {

static int64_t graph_bfs_blocks(int64_t n, int64_t n_sources) {
    const int64_t budget = (int64_t)1 << 30;                              // <= 1 GiB of per-workgroup search state
    int64_t blocks = budget / (8 * (n > 0 ? n : 1));
    if (blocks > n_sources) blocks = n_sources;
    if (blocks > 2048) blocks = 2048;
    return blocks < 1 ? 1 : blocks;
}

int64_t pp_graph_bfs_parts(int64_t n, int64_t n_sources) { return graph_bfs_blocks(n, n_sources); }

size_t pp_graph_bfs_ws_bytes(int64_t n, int64_t n_sources) {
    return pp::align_up((size_t)graph_bfs_blocks(n, n_sources) * 2 * (size_t)(n > 0 ? n : 1) * sizeof(int32_t));
}

int pp_graph_bfs(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t m, const int64_t* sources, int64_t n_sources, int32_t* dist,
                 int32_t* pred, int64_t* reach_in, int64_t* dist_in, int64_t* totals, void* ws, size_t ws_bytes, pp_stream_t stream) {
    PP_REQUIRE(m >= 0 && n >= 0 && n_sources >= 0, PP_ERR_ARG, "pp_graph_bfs: negative size");
    PP_REQUIRE(m <= (int64_t)0x7fffffff && n <= (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_bfs: size >= 2^31");
    PP_REQUIRE((reach_in == nullptr) == (dist_in == nullptr), PP_ERR_ARG, "pp_graph_bfs: reach_in and dist_in come together");
    PP_REQUIRE(ws_bytes >= pp_graph_bfs_ws_bytes(n, n_sources), PP_ERR_WORKSPACE, "pp_graph_bfs: workspace too small");
    if (n == 0 || n_sources == 0) return PP_OK;
    pp::k_graph_bfs<<<(unsigned)graph_bfs_blocks(n, n_sources), pp::kBlock, 0, (hipStream_t)stream>>>(row_ptr, col, n, sources, n_sources, dist, pred,
                                                                                                      reach_in, dist_in, totals, (int32_t*)ws);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

static int64_t graph_betweenness_blocks(int64_t n, int64_t n_sources) {
    const int64_t budget = (int64_t)1 << 30;                              // workspace slice + the workgroup's row of `partial`
    int64_t blocks = budget / (int64_t)(pp::graph_bw_block_bytes(n) + 8 * (size_t)(n > 0 ? n : 1));
    if (blocks > n_sources) blocks = n_sources;
    if (blocks > 1024) blocks = 1024;
    return blocks < 1 ? 1 : blocks;
}

int64_t pp_graph_betweenness_parts(int64_t n, int64_t n_sources) { return graph_betweenness_blocks(n, n_sources); }

size_t pp_graph_betweenness_ws_bytes(int64_t n, int64_t n_sources) {
    return (size_t)graph_betweenness_blocks(n, n_sources) * pp::graph_bw_block_bytes(n);
}

int pp_graph_betweenness(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t m, const int64_t* sources, int64_t n_sources,
                         double* partial, int32_t* reached, void* ws, size_t ws_bytes, pp_stream_t stream) {
    PP_REQUIRE(m >= 0 && n >= 0 && n_sources >= 0, PP_ERR_ARG, "pp_graph_betweenness: negative size");
    PP_REQUIRE(m <= (int64_t)0x7fffffff && n <= (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_betweenness: size >= 2^31");
    PP_REQUIRE(ws_bytes >= pp_graph_betweenness_ws_bytes(n, n_sources), PP_ERR_WORKSPACE, "pp_graph_betweenness: workspace too small");
    if (n == 0 || n_sources == 0) return PP_OK;
    pp::k_graph_betweenness<<<(unsigned)graph_betweenness_blocks(n, n_sources), pp::kBlock, 0, (hipStream_t)stream>>>(
        row_ptr, col, n, sources, n_sources, partial, reached, (char*)ws, pp::graph_bw_block_bytes(n));
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
