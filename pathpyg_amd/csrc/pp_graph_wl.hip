// pathpyg_amd — colour refinement (1-dimensional Weisfeiler-Leman) of a static Graph on its CSR.
//
// Reference: WeisfeilerLeman_test, src/pathpyG/algorithms/weisfeiler_leman.py:8-75 (every round builds one Python string per node out of a
// successors() call and the sorted labels of the successors, and numbers the strings through a dict).  Here a round is integer work on the
// device.  A node's signature is (own colour, multiset of the colours of its STORED successors): parallel edges count with their multiplicity,
// a self-loop contributes the node's own colour, predecessors play no part.  Nodes with equal signatures form a class; the classes are
// numbered 0 .. k-1 by the first occurrence of a member in `order`.
//   1. keys    : key[e] = row(e) * (k + 1) + colour[col[e]] (k = the current class count; a column outside [0, n) is not dereferenced and
//                counts as the colour k), one stable radix sort of the m keys (pp_sort.hip).  The row is the major part, so row v's sorted
//                colour sequence lies where its entries lay: sorted[row_ptr[v] .. row_ptr[v + 1]) - v * (k + 1).
//   2. signature: per node (own colour << 31 | degree, h1 >> 1 & mask, h2 >> 1 & mask), h1 and h2 two 64-bit sums of mixed colours
//                (a sum: the partial sums of lanes and waves fold in any shape to the same word).
//   3. groups  : nodes with equal signature words, by the lexicographic unique rows of pp_aggregate.hip.  The hash only SPEEDS UP grouping:
//   4. verify  : per group the unresolved node of smallest rank is elected (atomicMin on the rank); every unresolved node compares own
//                colour, degree and the sorted row, element by element, with the elected node's.  Equal: it joins that node's class.
//                Different: it stays unresolved and takes part in the group's next election.  Passes repeat until nobody is unresolved — one
//                pass with a working hash, more with mask = 0, the exact classes either way.
//   5. numbers : the elected nodes are flagged at their rank, the flags are scanned, a node's new colour is the scan at its class's rank.
// Work split of 2 and 4 (pp_rows.h): a row belongs to a GROUP of `width` lanes (a power of two, 1 .. 64, chosen from the mean
// degree); a row of heavy_min entries or more is left to a second launch with a whole workgroup per row.  The list of heavy rows is made
// once; its order depends on scheduling, no output does: every node writes its own words, elections are integer atomicMin, sums are integer.
// The round loop is a HOST loop over launches (as in pp_graph_components.hip) with one read-back per verify pass: {unresolved, classes}.
// Rounds are bounded by n + 1 (every round but the last adds a class).  No floating point anywhere.
#include <chrono>

#include "pp_common.h"
#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {

struct WlArgs {
    const int64_t* row_ptr;        // [n + 1]
    const uint64_t* sorted;        // [m] the sorted keys of this round
    const int64_t* colour;         // [n] the colours the round starts from
    int64_t n, m, k1;              // k1 = class count + 1: the multiplier of the row in a key
    uint64_t mask;
    int64_t* sig;                  // [n, 3]
    const int64_t* group;          // [n] group of equal signature words
    const uint32_t *rank, *node_of_rank, *rep_rank;
    int32_t* class_rep;            // [n] -1: unresolved, else the elected node of the class
    int32_t* flag;                 // [n] by rank: 1 where the node of that rank was elected
    int64_t* results;              // [0] somebody is still unresolved
    const uint32_t* heavy_list;
    int64_t heavy_count, heavy_min;
    int trust;                     // verify without comparing: the groups are exact already (round 0: groups of equal initial colour)
};

__device__ __forceinline__ uint64_t wl_mix1(uint64_t x) {                               // (the finaliser of splitmix64)
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t wl_mix2(uint64_t x) {                               // (the finaliser of MurmurHash3)
    x ^= 0xD6E8FEB86659FD93ull;
    x = (x ^ (x >> 33)) * 0xFF51AFD7ED558CCDull;
    x = (x ^ (x >> 33)) * 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}

// lane `sub` of `width` adds every width-th colour of row v
__device__ __forceinline__ void wl_hash_row(const WlArgs& a, int64_t v, int64_t lo, int64_t hi, int sub, int width, uint64_t& h1, uint64_t& h2) {
    const uint64_t base = (uint64_t)v * (uint64_t)a.k1;
    for (int64_t i = lo + sub; i < hi; i += width) {
        const uint64_t c = a.sorted[i] - base;
        h1 += wl_mix1(c);
        h2 += wl_mix2(c);
    }
}

__device__ __forceinline__ void wl_put_sig(const WlArgs& a, int64_t v, int64_t deg, uint64_t h1, uint64_t h2) {
    a.sig[3 * v] = (a.colour[v] << 31) | deg;                                           // (colour < n < 2^31, deg <= m < 2^31)
    a.sig[3 * v + 1] = (int64_t)((h1 >> 1) & a.mask);                                   // (63 bits: the words stay non-negative int64)
    a.sig[3 * v + 2] = (int64_t)((h2 >> 1) & a.mask);
}

// does lane `sub` of `width` meet a difference between the sorted rows of v and r (equal degrees)?
__device__ __forceinline__ bool wl_rows_differ(const WlArgs& a, int64_t v, int64_t lo, int64_t hi, int64_t r, int64_t rlo, int sub, int width) {
    const uint64_t vb = (uint64_t)v * (uint64_t)a.k1, rb = (uint64_t)r * (uint64_t)a.k1;
    for (int64_t i = sub; i < hi - lo; i += width)
        if (a.sorted[lo + i] - vb != a.sorted[rlo + i] - rb) return true;
    return false;
}

// the elected node of v's group, or -1 if the election's word is not a rank (never after k_wl_elect)
__device__ __forceinline__ int64_t wl_elected(const WlArgs& a, int64_t v) {
    const int64_t g = a.group[v];
    if ((uint64_t)g >= (uint64_t)a.n) return -1;
    const uint32_t rr = a.rep_rank[g];
    if ((uint64_t)rr >= (uint64_t)a.n) return -1;
    const uint32_t r = a.node_of_rank[rr];
    return (uint64_t)r < (uint64_t)a.n ? (int64_t)r : -1;
}

__device__ __forceinline__ void wl_resolve(const WlArgs& a, int64_t v, int64_t r, bool same) {
    const uint32_t rk = a.rank[v];
    if (same) a.class_rep[v] = (int32_t)r;
    else a.results[0] = 1;                                                              // (every writer stores the same word)
    if ((uint64_t)rk < (uint64_t)a.n) a.flag[rk] = same && r == v;
}

__global__ __launch_bounds__(kBlock) void k_wl_sig_groups(WlArgs a, int width) {
    const int sub = threadIdx.x & (width - 1);
    const int64_t per_block = kBlock / width, mine = threadIdx.x / width;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < a.n; base += (int64_t)gridDim.x * per_block) {       // (uniform in the workgroup)
        const int64_t v = base + mine;
        const bool live = v < a.n;
        uint64_t h1 = 0, h2 = 0;
        int64_t lo = 0, hi = 0;
        bool heavy = false;
        if (live) {
            row_span(a.row_ptr, v, a.m, lo, hi);
            heavy = hi - lo >= a.heavy_min;
            if (!heavy) wl_hash_row(a, v, lo, hi, sub, width, h1, h2);
        }
        group_sum(width, h1, h2);                                                       // (partners share the node: both are here)
        if (live && sub == 0 && !heavy) wl_put_sig(a, v, hi - lo, h1, h2);
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_sig_blocks(WlArgs a) {
    __shared__ uint64_t s_h1[kWavesPerBlock], s_h2[kWavesPerBlock];
    for (int64_t i = blockIdx.x; i < a.heavy_count; i += gridDim.x) {
        const int64_t v = a.heavy_list[i];
        if ((uint64_t)v >= (uint64_t)a.n) continue;                                     // (uniform in the workgroup)
        int64_t lo, hi;
        row_span(a.row_ptr, v, a.m, lo, hi);
        uint64_t h1 = 0, h2 = 0;
        wl_hash_row(a, v, lo, hi, (int)threadIdx.x, kBlock, h1, h2);
        h1 = wave_sum((unsigned long long)h1);
        h2 = wave_sum((unsigned long long)h2);
        if (lane_id() == 0) { s_h1[wave_id()] = h1; s_h2[wave_id()] = h2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t1 = 0, t2 = 0;
            for (int w = 0; w < kWavesPerBlock; ++w) { t1 += s_h1[w]; t2 += s_h2[w]; }
            wl_put_sig(a, v, hi - lo, t1, t2);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_elect(const int64_t* __restrict__ group, const uint32_t* __restrict__ rank,
                                                    const int32_t* __restrict__ class_rep, int64_t n, uint32_t* rep_rank) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const int64_t g = group[v];
        if (class_rep[v] >= 0 || (uint64_t)g >= (uint64_t)n) continue;
        const uint32_t r = rank[v];
        // few large groups: most lanes meet a word that is smaller already (an older value is a larger one: the test never skips wrongly)
        if (__hip_atomic_load(rep_rank + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > r) atomicMin(rep_rank + g, r);
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_verify_groups(WlArgs a, int width) {
    const int sub = threadIdx.x & (width - 1);
    const int64_t per_block = kBlock / width, mine = threadIdx.x / width;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < a.n; base += (int64_t)gridDim.x * per_block) {       // (uniform in the workgroup)
        const int64_t v = base + mine;
        int64_t lo = 0, hi = 0, r = -1;
        bool todo = v < a.n && a.class_rep[v] < 0, differ = false;
        if (todo) {
            row_span(a.row_ptr, v, a.m, lo, hi);
            todo = hi - lo < a.heavy_min;
        }
        if (todo) {
            r = wl_elected(a, v);
            if (r < 0) differ = true;
            else if (r != v && !a.trust) {
                int64_t rlo, rhi;
                row_span(a.row_ptr, r, a.m, rlo, rhi);
                differ = a.colour[r] != a.colour[v] || rhi - rlo != hi - lo || wl_rows_differ(a, v, lo, hi, r, rlo, sub, width);
            }
        }
        int bad = differ;
        for (int d = width >> 1; d > 0; d >>= 1) bad |= __shfl_xor(bad, d, kWave);
        if (todo && sub == 0) wl_resolve(a, v, r, !bad);
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_verify_blocks(WlArgs a) {
    __shared__ int s_bad;
    for (int64_t i = blockIdx.x; i < a.heavy_count; i += gridDim.x) {
        const int64_t v = a.heavy_list[i];
        if ((uint64_t)v >= (uint64_t)a.n || a.class_rep[v] >= 0) continue;              // (uniform in the workgroup: class_rep[v] is this workgroup's to write)
        if (threadIdx.x == 0) s_bad = 0;
        __syncthreads();
        int64_t lo, hi;
        row_span(a.row_ptr, v, a.m, lo, hi);
        const int64_t r = wl_elected(a, v);
        bool differ = false;
        if (r < 0) differ = true;
        else if (r != v && !a.trust) {
            int64_t rlo, rhi;
            row_span(a.row_ptr, r, a.m, rlo, rhi);
            differ = a.colour[r] != a.colour[v] || rhi - rlo != hi - lo || wl_rows_differ(a, v, lo, hi, r, rlo, (int)threadIdx.x, kBlock);
        }
        if (differ) s_bad = 1;
        __syncthreads();
        const bool same = s_bad == 0;
        __syncthreads();                                                                // (everybody has read s_bad before class_rep[v] changes and before the next row resets it)
        if (threadIdx.x == 0) wl_resolve(a, v, r, same);
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_recolour(const int32_t* __restrict__ class_rep, const uint32_t* __restrict__ rank,
                                                       const int32_t* __restrict__ pos, int64_t n, int64_t* __restrict__ colour_out) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const int32_t r = class_rep[v];
        int64_t c = 0;
        if ((uint32_t)r < (uint64_t)n) {
            const uint32_t rk = rank[r];
            if ((uint64_t)rk < (uint64_t)n) c = pos[rk];
        }
        colour_out[v] = c;
    }
}

// ------------------------------------------------------------------ set-up: ranks, the row of every entry, the heavy rows
__global__ __launch_bounds__(kBlock) void k_wl_ranks(const int64_t* __restrict__ order, int64_t n, uint32_t* __restrict__ rank,
                                                    uint32_t* __restrict__ node_of_rank) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const int64_t r = order ? order[v] : v;
        const bool ok = (uint64_t)r < (uint64_t)n;
        rank[v] = ok ? (uint32_t)r : 0xffffffffu;
        if (ok) node_of_rank[r] = (uint32_t)v;                                          // (a permutation: one writer per word; anything else is counted below)
    }
}

// results[2] += ranks that no node holds (node_of_rank was filled with 0xff before k_wl_ranks): 0 iff `order` is a permutation of 0 .. n-1
__global__ __launch_bounds__(kBlock) void k_wl_check_ranks(const uint32_t* __restrict__ node_of_rank, int64_t n, int64_t* results) {
    int64_t bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) bad += node_of_rank[r] == 0xffffffffu;
    bad = wave_sum(bad);
    if (lane_id() == 0 && bad) atomicAdd((unsigned long long*)&results[2], (unsigned long long)bad);
}

__global__ __launch_bounds__(kBlock) void k_wl_entry_rows(const int64_t* __restrict__ row_ptr, int64_t n, int64_t m, uint32_t* __restrict__ row_of) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        int64_t r = upper_bound_dev(row_ptr, (int64_t)0, n + 1, e) - 1;                 // the last row that starts at or before e
        r = r < 0 ? 0 : (r >= n ? n - 1 : r);
        row_of[e] = (uint32_t)r;
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_heavy_rows(const int64_t* __restrict__ row_ptr, int64_t n, int64_t m, int64_t heavy_min,
                                                         uint32_t* __restrict__ heavy_list, int64_t* results) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int64_t lo, hi;
        row_span(row_ptr, v, m, lo, hi);
        if (hi - lo >= heavy_min) heavy_list[atomicAdd((unsigned long long*)&results[3], 1ull)] = (uint32_t)v;        // (each node at most once: n entries)
    }
}

__global__ __launch_bounds__(kBlock) void k_wl_keys(const int64_t* __restrict__ col, const uint32_t* __restrict__ row_of,
                                                   const int64_t* __restrict__ colour, int64_t n, int64_t m, int64_t k1, uint64_t* __restrict__ keys) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t w = col[e];
        int64_t c = k1 - 1;
        if ((uint64_t)w < (uint64_t)n) {
            c = colour[w];
            c = c < 0 ? 0 : (c >= k1 ? k1 - 1 : c);
        }
        keys[e] = (uint64_t)row_of[e] * (uint64_t)k1 + (uint64_t)c;
    }
}

struct WlWs {
    uint32_t *row_of, *vals, *rank, *node_of_rank, *rep_rank, *heavy_list;
    uint64_t *keys, *sorted;
    int64_t *colour_b, *sig, *group, *results;
    int32_t *class_rep, *flag, *pos;
    void *sort, *scan, *unique;
    size_t sort_bytes, scan_bytes, unique_bytes, total;
};

static WlWs carve_wl(void* ws, int64_t n, int64_t m) {
    Arena a(ws, 0);
    WlWs w{};
    w.results = a.take<int64_t>(8);
    w.row_of = a.take<uint32_t>(m);
    w.vals = a.take<uint32_t>(m);
    w.keys = a.take<uint64_t>(m);
    w.sorted = a.take<uint64_t>(m);
    w.rank = a.take<uint32_t>(n);
    w.node_of_rank = a.take<uint32_t>(n);
    w.rep_rank = a.take<uint32_t>(n);
    w.heavy_list = a.take<uint32_t>(n);
    w.colour_b = a.take<int64_t>(n);
    w.sig = a.take<int64_t>(3 * n);
    w.group = a.take<int64_t>(n);
    w.class_rep = a.take<int32_t>(n);
    w.flag = a.take<int32_t>(n);
    w.pos = a.take<int32_t>(n + 1);
    w.sort_bytes = sort_ws_bytes(m, 8);
    w.sort = a.take<char>((int64_t)w.sort_bytes);
    w.scan_bytes = scan_ws_bytes(n);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.unique_bytes = pp_unique_rows_ws_bytes(n);
    w.unique = a.take<char>((int64_t)w.unique_bytes);
    w.total = a.used;
    return w;
}

struct WlClock {
    double* seconds;               // nullptr: nothing is timed and nothing waits
    hipStream_t st;
    std::chrono::steady_clock::time_point t0;
    int start() {
        if (!seconds) return PP_OK;
        PP_HIP(hipStreamSynchronize(st));
        t0 = std::chrono::steady_clock::now();
        return PP_OK;
    }
    int stop(int slot) {
        if (!seconds) return PP_OK;
        PP_HIP(hipStreamSynchronize(st));
        seconds[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return PP_OK;
    }
};

// elect, verify, number until nobody is unresolved; `colour_out` and host[1] = the class count are valid when it returns PP_OK
static int wl_resolve_classes(WlArgs& a, const WlWs& w, int width, int64_t* colour_out, int64_t* host, int64_t* passes, hipStream_t st) {
    const int64_t n = a.n;
    const unsigned gn = capped_grid(n, kBlock);
    PP_HIP(hipMemsetAsync(w.class_rep, 0xff, (size_t)n * sizeof(int32_t), st));         // -1: unresolved
    *passes = 0;
    for (;;) {
        PP_REQUIRE(*passes < n, PP_ERR_HIP, "pp_graph_wl_refine: nodes are still unresolved after n = %lld verify passes", (long long)n);
        ++*passes;
        PP_HIP(hipMemsetAsync(w.results, 0, 2 * sizeof(int64_t), st));
        PP_HIP(hipMemsetAsync(w.rep_rank, 0xff, (size_t)n * sizeof(uint32_t), st));
        k_wl_elect<<<gn, kBlock, 0, st>>>(w.group, w.rank, w.class_rep, n, w.rep_rank);
        PP_LAUNCH_CHECK();
        k_wl_verify_groups<<<capped_grid(n, kBlock / width), kBlock, 0, st>>>(a, width);
        PP_LAUNCH_CHECK();
        if (a.heavy_count > 0) {
            k_wl_verify_blocks<<<capped_grid(a.heavy_count, 1), kBlock, 0, st>>>(a);
            PP_LAUNCH_CHECK();
        }
        const int rc = exclusive_scan<int32_t, int32_t>(w.flag, n, w.pos, true, w.results + 1, w.scan, w.scan_bytes, st);
        if (rc != PP_OK) return rc;
        k_wl_recolour<<<gn, kBlock, 0, st>>>(w.class_rep, w.rank, w.pos, n, colour_out);
        PP_LAUNCH_CHECK();
        PP_HIP(hipMemcpyAsync(host, w.results, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        if (host[0] == 0) return PP_OK;
    }
}

}  // namespace pp

extern "C" {

int64_t pp_graph_wl_heavy_min(void) { return pp::kHeavyMinDefault; }

size_t pp_graph_wl_ws_bytes(int64_t n, int64_t m) { return pp::carve_wl(nullptr, n > 0 ? n : 0, m > 0 ? m : 0).total; }

int pp_graph_wl_refine(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t m, const int64_t* initial, const int64_t* order,
                       int64_t max_rounds, int64_t hash_mask, int group, int64_t heavy_min, int64_t* colours, int64_t* counts, int64_t* passes,
                       int64_t stats_cap, int64_t* rounds_out, double* seconds, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(m >= 0 && n >= 0, PP_ERR_ARG, "pp_graph_wl_refine: negative size");
    PP_REQUIRE(m < (int64_t)0x7fffffff && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_wl_refine: size >= 2^31 - 1");
    PP_REQUIRE(counts && passes && rounds_out && stats_cap >= 2, PP_ERR_ARG, "pp_graph_wl_refine: counts, passes (two entries or more) and rounds_out are required");
    PP_REQUIRE(n == 0 || (colours && row_ptr), PP_ERR_ARG, "pp_graph_wl_refine: colours and row_ptr are required");
    PP_REQUIRE(m == 0 || col, PP_ERR_ARG, "pp_graph_wl_refine: col is required");
    PP_REQUIRE(row_width_ok(group) && heavy_min >= 0, PP_ERR_ARG, "pp_graph_wl_refine: group must be 0 or a power of two up to 64");
    PP_REQUIRE(ws_bytes >= pp_graph_wl_ws_bytes(n, m), PP_ERR_WORKSPACE, "pp_graph_wl_refine: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (seconds) seconds[0] = seconds[1] = seconds[2] = 0.0;
    *rounds_out = 0;
    counts[0] = passes[0] = 0;
    if (n == 0) {                                                                       // no classes, and a round finds none either
        if (max_rounds != 0) { counts[1] = passes[1] = 0; *rounds_out = 1; }
        return PP_OK;
    }
    const WlWs w = carve_wl(ws, n, m);
    const int width = row_width(group, n, m);
    const unsigned gn = capped_grid(n, kBlock), gm = capped_grid(m, kBlock);
    int64_t host[4] = {0, 0, 0, 0};
    WlClock clock{seconds, st, {}};

    // set-up: ranks (checked), the row of every entry, the heavy rows; one read-back
    PP_HIP(hipMemsetAsync(w.results, 0, 8 * sizeof(int64_t), st));
    PP_HIP(hipMemsetAsync(w.node_of_rank, 0xff, (size_t)n * sizeof(uint32_t), st));
    k_wl_ranks<<<gn, kBlock, 0, st>>>(order, n, w.rank, w.node_of_rank);
    PP_LAUNCH_CHECK();
    if (order) {
        k_wl_check_ranks<<<gn, kBlock, 0, st>>>(w.node_of_rank, n, w.results);
        PP_LAUNCH_CHECK();
    }
    WlArgs a{};
    a.row_ptr = row_ptr; a.sorted = w.sorted; a.n = n; a.m = m; a.mask = (uint64_t)hash_mask; a.sig = w.sig; a.group = w.group;
    a.rank = w.rank; a.node_of_rank = w.node_of_rank; a.rep_rank = w.rep_rank; a.class_rep = w.class_rep; a.flag = w.flag;
    a.results = w.results; a.heavy_list = w.heavy_list; a.heavy_min = heavy_min > 0 ? heavy_min : kHeavyMinDefault;
    if (m > 0) {
        k_wl_entry_rows<<<gm, kBlock, 0, st>>>(row_ptr, n, m, w.row_of);
        PP_LAUNCH_CHECK();
        k_wl_heavy_rows<<<gn, kBlock, 0, st>>>(row_ptr, n, m, a.heavy_min, w.heavy_list, w.results);
        PP_LAUNCH_CHECK();
    }
    PP_HIP(hipMemcpyAsync(host, w.results, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    PP_REQUIRE(host[2] == 0, PP_ERR_ARG, "pp_graph_wl_refine: order is not a permutation of 0 .. n - 1");
    a.heavy_count = host[3] > n ? n : host[3];

    // round 0: the classes of equal initial colour, numbered by first occurrence
    int64_t *cur = colours, *nxt = w.colour_b;
    if (initial) {
        int rc = minmax_i64(initial, n, w.results + 4, st);
        if (rc != PP_OK) return rc;
        PP_HIP(hipMemcpyAsync(host, w.results + 4, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        rc = pp_unique_rows_count(initial, n, 1, host[0], host[1], w.group, w.unique, w.unique_bytes, stream);
        if (rc != PP_OK) return rc;
        a.trust = 1;
        a.colour = initial;
        a.k1 = 1;
        const int64_t heavy = a.heavy_count;
        a.heavy_count = 0;                                                              // (nothing is compared: every row is a light one)
        const int64_t heavy_min_set = a.heavy_min;
        a.heavy_min = (int64_t)0x7fffffff;
        rc = wl_resolve_classes(a, w, width, cur, host, &passes[0], st);
        if (rc != PP_OK) return rc;
        a.heavy_count = heavy;
        a.heavy_min = heavy_min_set;
        a.trust = 0;
        counts[0] = host[1];
    } else {
        PP_HIP(hipMemsetAsync(cur, 0, (size_t)n * sizeof(int64_t), st));
        counts[0] = 1;
    }

    int64_t rounds = 0;
    while (max_rounds < 0 || rounds < max_rounds) {
        PP_REQUIRE(rounds <= n, PP_ERR_HIP, "pp_graph_wl_refine: the class count still grows after n + 1 = %lld rounds", (long long)(n + 1));
        PP_REQUIRE(rounds + 2 <= stats_cap, PP_ERR_ARG, "pp_graph_wl_refine: more than stats_cap - 1 = %lld rounds", (long long)(stats_cap - 1));
        const int64_t k = counts[rounds];
        a.k1 = k + 1;
        a.colour = cur;
        int rc = clock.start();
        if (rc != PP_OK) return rc;
        if (m > 0) {
            k_wl_keys<<<gm, kBlock, 0, st>>>(col, w.row_of, cur, n, m, a.k1, w.keys);
            PP_LAUNCH_CHECK();
            const int bits = bits_for((uint64_t)n * (uint64_t)a.k1 - 1);
            rc = sort_pairs<uint64_t>(w.keys, nullptr, w.sorted, w.vals, m, 0, bits, w.sort, w.sort_bytes, st);
            if (rc != PP_OK) return rc;
        }
        if ((rc = clock.stop(0)) != PP_OK || (rc = clock.start()) != PP_OK) return rc;
        k_wl_sig_groups<<<capped_grid(n, kBlock / width), kBlock, 0, st>>>(a, width);
        PP_LAUNCH_CHECK();
        if (a.heavy_count > 0) {
            k_wl_sig_blocks<<<capped_grid(a.heavy_count, 1), kBlock, 0, st>>>(a);
            PP_LAUNCH_CHECK();
        }
        if ((rc = clock.stop(1)) != PP_OK || (rc = clock.start()) != PP_OK) return rc;
        rc = pp_unique_rows_count(w.sig, n, 3, 0, INT64_MAX, w.group, w.unique, w.unique_bytes, stream);
        if (rc != PP_OK) return rc;
        if ((rc = clock.stop(2)) != PP_OK || (rc = clock.start()) != PP_OK) return rc;
        rc = wl_resolve_classes(a, w, width, nxt, host, &passes[rounds + 1], st);
        if (rc != PP_OK) return rc;
        if ((rc = clock.stop(1)) != PP_OK) return rc;
        ++rounds;
        counts[rounds] = host[1];
        int64_t* t = cur; cur = nxt; nxt = t;
        if (counts[rounds] == counts[rounds - 1]) break;                                // stable: the same partition, the same numbers
    }
    *rounds_out = rounds;
    if (cur != colours) PP_HIP(hipMemcpyAsync(colours, cur, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return PP_OK;
}

}  // extern "C"
