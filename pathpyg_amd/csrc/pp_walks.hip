// pathpyg_amd — random walks on a Graph or on a layer of a MultiOrderModel, sampled on the device (no reference counterpart in the snapshot
// this package follows; upstream pathpyG grew a `processes` package for it, whose sampling is a Python loop per step).
//
// W independent pointer chases: one lane per walk, its state in registers, the step loop inside the kernel.  Every random word is the
// Philox word of (seed, tag, stream, index) of pp_philox.h — PP_RG_TAG_WALK_START (stream = the rejection attempt, index = the walk) and
// PP_RG_TAG_WALK_STEP (stream = the step, index = the walk) — so a walk is a pure function of (seed, graph, weights, arguments), whichever
// lane of whichever grid works it.  A uniform is x = (double)(word >> 11) * 2^-53; everything between x and an index is float64 with ONE
// rounded operation per line of the header's contract (contraction is off in this file, and the products and differences are spelled as
// __dmul_rn / __dsub_rn), which tests/cpu_ops_walks.py restates with Python floats.
//
// What bounds the walk kernel: per step a chain of DEPENDENT random reads — row_ptr[v], row_ptr[v + 1] (one line, mostly), then about
// log2(deg) reads of cum[] for the bisection, then col[j]; total[v] does not depend on the pointers and is in flight beside them.  Nothing
// but other waves hides those misses, so the kernel keeps its registers low enough for 8 waves per SIMD (DESIGN.md "Random walks").
#include "pp_common.h"
#include "pp_internal.h"
#include "pp_philox.h"
#include "pp_rows.h"

#pragma clang fp contract(off)

namespace pp {

constexpr int kWalkBlockLog2 = 10;                      // nodes per block of the start table
constexpr int64_t kWalkBlock = (int64_t)1 << kWalkBlockLog2;
constexpr int64_t kWalkLimit = 0x7fffffff;              // sizes stay below 2^31 - 1
constexpr int kWalkMaxAttempts = 4096;                  // pp_rg_draws' rule: a bounded draw is rejected with probability < 1/2 per attempt

enum { kStartGiven = 0, kStartWeighted = 1, kStartUniform = 2 };

__device__ __forceinline__ double walk_uniform(uint64_t word) { return __dmul_rn((double)(word >> 11), 0x1.0p-53); }

// cum[j] = the left-to-right running sum of row v's weights up to entry j (row-local), total[v] = the row's last cum (0: empty row)
template <typename WT>
__global__ __launch_bounds__(kBlock) void k_walk_table(const int64_t* __restrict__ row_ptr, int64_t n, int64_t m, const WT* __restrict__ weight,
                                                      double* __restrict__ cum, double* __restrict__ total, int32_t* __restrict__ bad) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int64_t lo, hi;
        row_span(row_ptr, v, m, lo, hi);
        double s = 0.0;
        bool wrong = false;
        for (int64_t j = lo; j < hi; ++j) {
            const double w = weight ? (double)weight[j] : 1.0;
            wrong |= !(w >= 0.0) || w > 1.7976931348623157e308;                        // negative, NaN or infinite
            s += w;
            cum[j] = s;
        }
        total[v] = s;
        wrong |= s > 1.7976931348623157e308;                                           // finite weights whose sum is not
        if (wrong) bad[0] = 1;                                                        // (every lane that finds one stores the same 1)
    }
}

// bcum[i] = the running sum of total[] inside i's block of 1024 nodes; one lane per block
__global__ __launch_bounds__(kBlock) void k_walk_start_blocks(const double* __restrict__ total, int64_t n, int64_t blocks, double* __restrict__ bcum,
                                                             double* __restrict__ B) {
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < blocks; b += (int64_t)gridDim.x * kBlock) {
        const int64_t first = b << kWalkBlockLog2, end = first + kWalkBlock < n ? first + kWalkBlock : n;
        double s = 0.0;
        for (int64_t i = first; i < end; ++i) {
            s += total[i];
            bcum[i] = s;
        }
        B[b] = s;                                                                      // the block's total; k_walk_start_fold makes it a running sum
    }
}

__global__ void k_walk_start_fold(int64_t blocks, double* __restrict__ B) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int64_t b = 0; b < blocks; ++b) {
            s += B[b];
            B[b] = s;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_walk_positive_flag(const double* __restrict__ total, int64_t n, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) flag[v] = total[v] > 0.0;
}

__global__ __launch_bounds__(kBlock) void k_walk_positive_list(const int64_t* __restrict__ pos, int64_t n, int64_t cap, int32_t* __restrict__ list) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const int64_t p = pos[v];
        if (pos[v + 1] > p && p >= 0 && p < cap) list[p] = (int32_t)v;
    }
}

struct WalkStart {
    const int64_t* given;        // kStartGiven: [W]
    const double* bcum;          // kStartWeighted: [n]
    const double* B;             // kStartWeighted: [blocks]
    const int32_t* list;         // kStartUniform: [list_len]
    int64_t blocks, list_len;
};

// the start node of walk w, or -1 (a given start outside [0, n); tables that hold no node)
template <int MODE>
__device__ __forceinline__ int64_t walk_start(const WalkStart& s, const double* __restrict__ total, int64_t n, uint32_t k0, uint32_t k1, int64_t w) {
    if (MODE == kStartGiven) {
        const int64_t v = s.given[w];
        return (uint64_t)v < (uint64_t)n ? v : -1;
    }
    if (MODE == kStartUniform) {
        if (s.list_len <= 0) return -1;
        const uint64_t N = (uint64_t)s.list_len, thr = (0 - N) % N;
        uint64_t word = 0;
        for (uint64_t a = 0; a < kWalkMaxAttempts; ++a) {
            word = rg_word(k0, k1, PP_RG_TAG_WALK_START, a, (uint64_t)w);
            if (word * N >= thr) break;
        }
        const int64_t v = s.list[__umul64hi(word, N)];
        return (uint64_t)v < (uint64_t)n ? v : -1;
    }
    if (s.blocks <= 0) return -1;
    const double x = walk_uniform(rg_word(k0, k1, PP_RG_TAG_WALK_START, 0, (uint64_t)w));
    const double target = __dmul_rn(x, s.B[s.blocks - 1]);
    int64_t b = upper_bound_dev(s.B, (int64_t)0, s.blocks, target);                    // the first block with B[b] > target
    if (b >= s.blocks) b = s.blocks - 1;                                               // (target < B[last] for a finite positive normal B[last])
    const double t2 = __dsub_rn(target, b ? s.B[b - 1] : 0.0);
    const int64_t first = b << kWalkBlockLog2, end = first + kWalkBlock < n ? first + kWalkBlock : n;
    int64_t v = upper_bound_dev(s.bcum, first, end, t2);                               // the first node of the block with bcum > t2
    if (v >= end) {                                                                    // rounding: the block's last node with a positive total
        for (v = end - 1; v >= first && !(total[v] > 0.0); --v) {}
        if (v < first) return -1;
    }
    return v;
}

// nodes [steps + 1, W] (step-major: the stores of a wave at one step are contiguous), -1 after a walk's end; lengths [W] in edges.  One
// instance per start mode: the tables of the other modes take no scalar registers (with all of them the kernel needed more than the 96 that
// 8 waves per SIMD leave a wave)
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_walk_run(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col, const double* __restrict__ cum,
                                                    const double* __restrict__ total, int64_t n, int64_t m, int64_t W, int64_t steps, uint32_t k0,
                                                    uint32_t k1, WalkStart start, int32_t* __restrict__ nodes, int32_t* __restrict__ lengths) {
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < W; w += (int64_t)gridDim.x * kBlock) {
        int64_t v = walk_start<MODE>(start, total, n, k0, k1, w);
        int32_t* out = nodes + w;
        *out = (int32_t)v;
        int64_t t = 0;
        if (v >= 0) {
            for (; t < steps; ++t) {
                const double T = total[v];                                             // (independent of the pointers: in flight beside them)
                int64_t lo, hi;
                row_span(row_ptr, v, m, lo, hi);
                if (hi <= lo || !(T > 0.0)) break;
                const double target = __dmul_rn(walk_uniform(rg_word(k0, k1, PP_RG_TAG_WALK_STEP, (uint64_t)t, (uint64_t)w)), T);
                const int64_t j = upper_bound_dev(cum, lo, hi, target);                // the smallest j of the row with cum[j] > target
                if (j >= hi) break;                                                    // (never for a finite positive normal T: target < T)
                const int64_t u = col[j];
                if ((uint64_t)u >= (uint64_t)n) break;
                v = u;
                out += W;
                *out = (int32_t)v;
            }
        }
        lengths[w] = (int32_t)t;
        for (int64_t r = t; r < steps; ++r) {
            out += W;
            *out = -1;
        }
    }
}

// keep[w] = the walk has an edge; count[w] = its first-order nodes (order + length) if so, else 0
__global__ __launch_bounds__(kBlock) void k_walk_pack_count(const int32_t* __restrict__ lengths, int64_t W, int64_t steps, int64_t order,
                                                           int32_t* __restrict__ keep, int32_t* __restrict__ count) {
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < W; w += (int64_t)gridDim.x * kBlock) {
        int64_t len = lengths[w];
        len = len < 0 ? 0 : (len > steps ? steps : len);
        keep[w] = len > 0;
        count[w] = len > 0 ? (int32_t)(order + len) : 0;
    }
}

// one lane per walk: reads of the step-major buffer are contiguous in the wave, each lane writes its own run of the packed store
__global__ __launch_bounds__(kBlock) void k_walk_pack_fill(const int32_t* __restrict__ nodes, const int32_t* __restrict__ lengths, int64_t W, int64_t steps,
                                                          int64_t order, int64_t n, const int64_t* __restrict__ node_sequence,
                                                          const int64_t* __restrict__ offset, const int64_t* __restrict__ rank, int64_t P, int64_t kept,
                                                          int64_t* __restrict__ seq_out, int64_t* __restrict__ edge_src, int64_t* __restrict__ edge_dst,
                                                          int64_t* __restrict__ dag_nodes, int64_t* __restrict__ dag_edges, float* __restrict__ dag_weight) {
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < W; w += (int64_t)gridDim.x * kBlock) {
        int64_t len = lengths[w];
        len = len < 0 ? 0 : (len > steps ? steps : len);
        if (len == 0) continue;
        const int64_t o = offset[w], r = rank[w], c = order + len;
        if (o < 0 || o + c > P || r < 0 || r >= kept) continue;                        // (a write never leaves the outputs)
        dag_nodes[r] = c;
        dag_edges[r] = c - 1;
        dag_weight[r] = 1.f;
        int64_t u = nodes[w];
        const bool ok0 = (uint64_t)u < (uint64_t)n;
        for (int64_t i = 0; i < order; ++i) seq_out[o + i] = ok0 ? node_sequence[u * order + i] : -1;
        for (int64_t t = 1; t <= len; ++t) {
            u = nodes[t * W + w];
            seq_out[o + order + t - 1] = (uint64_t)u < (uint64_t)n ? node_sequence[u * order + order - 1] : -1;
        }
        const int64_t e = o - r;                                                       // every kept walk before this one left one edge less than nodes
        for (int64_t i = 0; i + 1 < c; ++i) {
            edge_src[e + i] = o + i;
            edge_dst[e + i] = o + i + 1;
        }
    }
}

static unsigned walk_grid(int64_t items) {
    int64_t g = ceil_div(items > 0 ? items : 1, kBlock);
    const int64_t share = shared_grid(kMaxGrid);
    if (g > share) g = share;
    note_persistent_grid(g);
    return (unsigned)g;
}

}  // namespace pp

extern "C" {

int pp_walk_check_sizes(int64_t n, int64_t m, int64_t walks, int64_t steps, int64_t order) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && m >= 0 && walks >= 0 && steps >= 0 && order >= 1, PP_ERR_ARG, "pp_walk: negative size, or order < 1");
    PP_REQUIRE(n < kWalkLimit && m < kWalkLimit, PP_ERR_TOO_LARGE, "pp_walk: 2^31 - 1 nodes or entries, or more");
    PP_REQUIRE(steps < kWalkLimit && order < kWalkLimit && walks < kWalkLimit, PP_ERR_TOO_LARGE, "pp_walk: 2^31 - 1 walks, steps or columns, or more");
    PP_REQUIRE(walks * (steps + order) < kWalkLimit, PP_ERR_TOO_LARGE, "pp_walk: walks * (steps + order) reaches 2^31 - 1");   // (< 2^63: each below 2^31)
    return PP_OK;
}

int pp_walk_table(const int64_t* row_ptr, int64_t n, int64_t m, const void* weight, int weight_dtype, double* cum, double* total, int32_t* bad,
                  pp_stream_t stream) {
    using namespace pp;
    const int rc = pp_walk_check_sizes(n, m, 0, 0, 1);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(weight_dtype == PP_F32 || weight_dtype == PP_F64, PP_ERR_ARG, "pp_walk_table: weights are float32 or float64");
    PP_REQUIRE(bad && (n == 0 || (row_ptr && total)) && (m == 0 || cum), PP_ERR_ARG, "pp_walk_table: null pointer");
    PP_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), (hipStream_t)stream));
    if (n == 0) return PP_OK;
    if (weight_dtype == PP_F32)
        k_walk_table<float><<<walk_grid(n), kBlock, 0, (hipStream_t)stream>>>(row_ptr, n, m, (const float*)weight, cum, total, bad);
    else
        k_walk_table<double><<<walk_grid(n), kBlock, 0, (hipStream_t)stream>>>(row_ptr, n, m, (const double*)weight, cum, total, bad);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int64_t pp_walk_start_blocks(int64_t n) { return n > 0 ? (n + pp::kWalkBlock - 1) >> pp::kWalkBlockLog2 : 0; }

int pp_walk_start_table(const double* total, int64_t n, double* bcum, double* block_cum, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0, PP_ERR_ARG, "pp_walk_start_table: negative size");
    PP_REQUIRE(n < kWalkLimit, PP_ERR_TOO_LARGE, "pp_walk_start_table: 2^31 - 1 nodes or more");
    PP_REQUIRE(n == 0 || (total && bcum && block_cum), PP_ERR_ARG, "pp_walk_start_table: null pointer");
    if (n == 0) return PP_OK;
    const int64_t blocks = pp_walk_start_blocks(n);
    k_walk_start_blocks<<<walk_grid(blocks), kBlock, 0, (hipStream_t)stream>>>(total, n, blocks, bcum, block_cum);
    PP_LAUNCH_CHECK();
    k_walk_start_fold<<<1, kWave, 0, (hipStream_t)stream>>>(blocks, block_cum);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_walk_positive_flag(const double* total, int64_t n, int32_t* flag, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && (n == 0 || (total && flag)), PP_ERR_ARG, "pp_walk_positive_flag: bad arguments");
    PP_REQUIRE(n < kWalkLimit, PP_ERR_TOO_LARGE, "pp_walk_positive_flag: 2^31 - 1 nodes or more");
    if (n == 0) return PP_OK;
    k_walk_positive_flag<<<walk_grid(n), kBlock, 0, (hipStream_t)stream>>>(total, n, flag);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_walk_positive_list(const int64_t* pos, int64_t n, int64_t count, int32_t* list, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && count >= 0 && count <= n && (n == 0 || pos) && (count == 0 || list), PP_ERR_ARG, "pp_walk_positive_list: bad arguments");
    PP_REQUIRE(n < kWalkLimit, PP_ERR_TOO_LARGE, "pp_walk_positive_list: 2^31 - 1 nodes or more");
    if (n == 0 || count == 0) return PP_OK;
    k_walk_positive_list<<<walk_grid(n), kBlock, 0, (hipStream_t)stream>>>(pos, n, count, list);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_walk_run(const int64_t* row_ptr, const int64_t* col, const double* cum, const double* total, int64_t n, int64_t m, int64_t walks, int64_t steps,
                int64_t order, int64_t seed, int start_mode, const int64_t* start_nodes, const double* bcum, const double* block_cum,
                const int32_t* positive, int64_t positive_count, int32_t* nodes, int32_t* lengths, pp_stream_t stream) {
    using namespace pp;
    const int rc = pp_walk_check_sizes(n, m, walks, steps, order);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(start_mode >= kStartGiven && start_mode <= kStartUniform, PP_ERR_ARG, "pp_walk_run: unknown start mode");
    PP_REQUIRE(positive_count >= 0 && positive_count <= n, PP_ERR_ARG, "pp_walk_run: bad start list length");
    if (walks == 0) return PP_OK;
    PP_REQUIRE(n >= 1, PP_ERR_ARG, "pp_walk_run: walks on a graph without nodes");
    PP_REQUIRE(row_ptr && total && (m == 0 || (col && cum)) && nodes && lengths, PP_ERR_ARG, "pp_walk_run: null pointer");
    PP_REQUIRE(start_mode != kStartGiven || start_nodes, PP_ERR_ARG, "pp_walk_run: no start nodes");
    PP_REQUIRE(start_mode != kStartWeighted || (bcum && block_cum), PP_ERR_ARG, "pp_walk_run: no start table");
    PP_REQUIRE(start_mode != kStartUniform || (positive && positive_count >= 1), PP_ERR_ARG, "pp_walk_run: no start list");
    WalkStart s{};
    s.given = start_nodes;
    s.bcum = bcum;
    s.B = block_cum;
    s.list = positive;
    s.blocks = pp_walk_start_blocks(n);
    s.list_len = positive_count;
    const unsigned grid = walk_grid(walks);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
    if (start_mode == kStartGiven)
        k_walk_run<kStartGiven><<<grid, kBlock, 0, (hipStream_t)stream>>>(row_ptr, col, cum, total, n, m, walks, steps, k0, k1, s, nodes, lengths);
    else if (start_mode == kStartWeighted)
        k_walk_run<kStartWeighted><<<grid, kBlock, 0, (hipStream_t)stream>>>(row_ptr, col, cum, total, n, m, walks, steps, k0, k1, s, nodes, lengths);
    else
        k_walk_run<kStartUniform><<<grid, kBlock, 0, (hipStream_t)stream>>>(row_ptr, col, cum, total, n, m, walks, steps, k0, k1, s, nodes, lengths);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_walk_pack_count(const int32_t* lengths, int64_t walks, int64_t steps, int64_t order, int32_t* keep, int32_t* count, pp_stream_t stream) {
    using namespace pp;
    const int rc = pp_walk_check_sizes(0, 0, walks, steps, order);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(walks == 0 || (lengths && keep && count), PP_ERR_ARG, "pp_walk_pack_count: null pointer");
    if (walks == 0) return PP_OK;
    k_walk_pack_count<<<walk_grid(walks), kBlock, 0, (hipStream_t)stream>>>(lengths, walks, steps, order, keep, count);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_walk_pack_fill(const int32_t* nodes, const int32_t* lengths, int64_t walks, int64_t steps, int64_t order, int64_t n,
                      const int64_t* node_sequence, const int64_t* offset, const int64_t* rank, int64_t positions, int64_t kept,
                      int64_t* seq_out, int64_t* edge_src, int64_t* edge_dst, int64_t* dag_num_nodes, int64_t* dag_num_edges, float* dag_weight,
                      pp_stream_t stream) {
    using namespace pp;
    const int rc = pp_walk_check_sizes(n, 0, walks, steps, order);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(positions >= 0 && kept >= 0 && kept <= walks && positions >= kept, PP_ERR_ARG, "pp_walk_pack_fill: bad output sizes");
    if (walks == 0 || kept == 0) return PP_OK;
    PP_REQUIRE(nodes && lengths && node_sequence && offset && rank && seq_out && edge_src && edge_dst && dag_num_nodes && dag_num_edges && dag_weight,
               PP_ERR_ARG, "pp_walk_pack_fill: null pointer");
    k_walk_pack_fill<<<walk_grid(walks), kBlock, 0, (hipStream_t)stream>>>(nodes, lengths, walks, steps, order, n, node_sequence, offset, rank, positions,
                                                                          kept, seq_out, edge_src, edge_dst, dag_num_nodes, dag_num_edges, dag_weight);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
