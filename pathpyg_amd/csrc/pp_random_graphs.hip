// pathpyg_amd — random graph models sampled on the device (reference src/pathpyG/algorithms/generative_models.py: Python loops over all
// n^2 pairs for G(n,p) and the block model, a set with two IndexMap lookups per draw for G(n,m)).
//
// The random stream is a PURE FUNCTION of (seed, arguments): Philox4x32-10 (Salmon et al., Random123) keyed by the 64-bit seed; the 128-bit
// counter is
//     c0, c1 : a 64-bit index (the draw inside a chunk; the draw / edge index elsewhere)
//     c2     : the low 32 bits of a stream (the chunk of a region; the rejection attempt of a bounded draw)
//     c3     : tag << 24 | stream bits 32 .. 55 (the high chunk bits; the repair round of Watts-Strogatz)
// and every use owns a tag (kTag*), so no two uses share a counter.  A draw is the 64-bit word x | y << 32 of one Philox block.  Everything
// between that word and an edge is integer arithmetic — tests/cpu_ops_generative.py restates it with Python ints, bit for bit.  Nothing
// depends on the grid: a chunk / draw / edge is worked by whichever lane meets it.
//
// Region sampler (G(n,p), block model): a Bernoulli(p) subset of the slot space [0, N) of a region of "rank space" (rectangle, square
// without its diagonal, strict lower triangle, lower triangle with diagonal), cut into chunks of 2^k slots with about CHUNK_EDGES expected
// edges.  One lane walks one chunk by geometric skips: slot += 1 + g, g = floor(-log2(u) * c), c = -1 / log2(1 - p).  -log2(u) of the
// 63-bit draw comes from count-leading-zeros and 40 square-and-compare steps on a Q1.63 mantissa (error <= 2^-40); c arrives with 32
// fraction bits (c < 2^32: p >= 2^-30), the product is taken in 128 bits, g < 2^38 and a slot < 2^63: nothing wraps.  count -> scan -> fill;
// the fill pass regenerates the streams and stages kRgStage edges per lane in LDS, which the workgroup copies out as full 128-byte runs.
#include "pp_common.h"
#include "pp_internal.h"
#include "pp_philox.h"

namespace pp {

constexpr int kRgFrac = 40;            // fraction bits of -log2(u)
constexpr int kRgStage = 16;           // edges a lane stages per copy round (16 x int64 = one 128-byte run per output row)
constexpr int kRgRegionWords = 8;      // int64 words of a region descriptor
constexpr int kRgMaxAttempts = 4096;   // a bounded draw is rejected with probability < 1/2 per attempt

enum { kRegRect = 0, kRegStrict = 1, kRegDiag = 2, kRegNoDiag = 3 };

// -log2(((w >> 1) + 1) / 2^63) with kRgFrac fraction bits, rounded up by less than 2^-40
__device__ __forceinline__ uint64_t rg_neglog2(uint64_t w) {
    const uint64_t v = (w >> 1) + 1;                                                    // 1 .. 2^63
    const int e = 63 - __clzll((long long)v);
    uint64_t x = v << (63 - e), frac = 0;                                               // Q1.63 in [2^63, 2^64)
    for (int i = 0; i < kRgFrac; ++i) {
        x = __umul64hi(x, x);                                                           // Q2.62
        if (x >> 63) frac = (frac << 1) | 1;
        else { frac <<= 1; x <<= 1; }
    }
    return ((uint64_t)(63 - e) << kRgFrac) - frac;
}

__device__ __forceinline__ uint64_t rg_skip(uint64_t w, uint64_t c) { return __umul64hi(rg_neglog2(w), c) >> (kRgFrac + 32 - 64); }

// row of slot s in a strict lower triangle (s = r (r - 1) / 2 + c, c < r): a sqrt estimate, made exact by integer comparison
__device__ __forceinline__ uint64_t rg_tri_row(uint64_t s) {
    uint64_t r = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)s)) * 0.5);
    if (r < 1) r = 1;
    while (r > 1 && ((r * (r - 1)) >> 1) > s) --r;
    while ((((r + 1) * r) >> 1) <= s) ++r;
    return r;
}

__device__ __forceinline__ void rg_decode(int kind, uint64_t cols, uint64_t s, uint64_t& r, uint64_t& c) {
    if (kind == kRegStrict || kind == kRegDiag) {
        const uint64_t t = rg_tri_row(s);
        c = s - ((t * (t - 1)) >> 1);
        r = kind == kRegDiag ? t - 1 : t;
    } else {
        const uint64_t d = cols > 0 ? cols : 1;
        r = s / d;
        c = s - r * d;
        if (kind == kRegNoDiag && c >= r) ++c;                                          // the column is shifted past the diagonal
    }
}

// unbiased draw below N (N >= 1): multiply-high, rejected while the low word lies under 2^64 mod N; the attempt is the stream's low word
__device__ __forceinline__ uint64_t rg_below(uint64_t N, uint32_t k0, uint32_t k1, uint32_t tag, uint64_t round, uint64_t index) {
    const uint64_t thr = (0 - N) % N;
    uint64_t w = 0;
    for (uint64_t a = 0; a < kRgMaxAttempts; ++a) {
        w = rg_word(k0, k1, tag, (round << 32) | a, index);
        if (w * N >= thr) break;
    }
    return __umul64hi(w, N);
}

struct RgRegion {
    uint64_t slot0, end, c, cols, row_off, col_off;
    int kind;
};

// the region of a chunk: the last descriptor whose first chunk is <= chunk (empty regions share their first chunk with the next one)
__device__ __forceinline__ RgRegion rg_region(const int64_t* __restrict__ reg, int R, int64_t chunk) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (reg[(int64_t)mid * kRgRegionWords] <= chunk) lo = mid; else hi = mid;
    }
    const int64_t* d = reg + (int64_t)lo * kRgRegionWords;
    RgRegion g;
    const uint64_t N = (uint64_t)d[1], local = (uint64_t)(chunk - d[0]);
    const int shift = (int)d[2];
    g.slot0 = local << shift;
    g.end = g.slot0 + ((uint64_t)1 << shift);
    if (g.end > N) g.end = N;
    if (g.slot0 > N) g.slot0 = N;
    g.c = (uint64_t)d[3];
    g.kind = (int)d[4];
    g.cols = (uint64_t)d[5];
    g.row_off = (uint64_t)d[6];
    g.col_off = (uint64_t)d[7];
    return g;
}

__global__ __launch_bounds__(kBlock) void k_rg_count(const int64_t* __restrict__ reg, int R, int64_t n_chunks, uint32_t k0, uint32_t k1, uint32_t tag,
                                                    int64_t* __restrict__ counts) {
    for (int64_t chunk = (int64_t)blockIdx.x * kBlock + threadIdx.x; chunk < n_chunks; chunk += (int64_t)gridDim.x * kBlock) {
        const RgRegion g = rg_region(reg, R, chunk);
        uint64_t next = g.slot0, j = 0;
        int64_t count = 0;
        for (;;) {
            const uint64_t slot = next + rg_skip(rg_word(k0, k1, tag, (uint64_t)chunk, j++), g.c);
            if (slot >= g.end) break;
            ++count;
            next = slot + 1;
        }
        counts[chunk] = count;
    }
}

// offsets: the exclusive scan of the counts ([n_chunks + 1]); rows / cols: [total]; perm (or nullptr): rank -> node, [n]
__global__ __launch_bounds__(kBlock) void k_rg_fill(const int64_t* __restrict__ reg, int R, int64_t n_chunks, uint32_t k0, uint32_t k1, uint32_t tag,
                                                   const int64_t* __restrict__ offsets, const int64_t* __restrict__ perm, int64_t n, int64_t total,
                                                   int64_t* __restrict__ rows, int64_t* __restrict__ cols) {
    __shared__ uint2 s_edge[kBlock][kRgStage + 1];
    __shared__ int64_t s_out[kBlock], s_lim[kBlock];
    __shared__ int s_cnt[kBlock];
    const int t = threadIdx.x, e = t & (kRgStage - 1);
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n_chunks; base += (int64_t)gridDim.x * kBlock) {       // (uniform in the workgroup)
        const int64_t chunk = base + t;
        bool done = chunk >= n_chunks;
        RgRegion g{};
        uint64_t next = 0, j = 0;
        int64_t out = 0, lim = 0;
        if (!done) {
            g = rg_region(reg, R, chunk);
            next = g.slot0;
            out = offsets[chunk];
            lim = offsets[chunk + 1];
            if (lim > total) lim = total;                                               // (a write never leaves the output)
            if (out < 0) out = lim;
        }
        for (;;) {
            int k = 0;
            while (!done && k < kRgStage) {
                const uint64_t slot = next + rg_skip(rg_word(k0, k1, tag, (uint64_t)chunk, j++), g.c);
                if (slot >= g.end) { done = true; break; }
                uint64_t r, c;
                rg_decode(g.kind, g.cols, slot, r, c);
                s_edge[t][k++] = make_uint2((uint32_t)(r + g.row_off), (uint32_t)(c + g.col_off));
                next = slot + 1;
            }
            s_cnt[t] = k;
            s_out[t] = out;
            s_lim[t] = lim;
            out += k;
            if (!__syncthreads_or(k > 0)) break;                                        // (the same answer in every lane)
#pragma unroll 4
            for (int i = 0; i < kRgStage; ++i) {                                        // 16 lanes per staged run: consecutive addresses
                const int seg = (t >> 4) + i * (kBlock / kRgStage);
                const int64_t idx = s_out[seg] + e;
                if (e < s_cnt[seg] && idx < s_lim[seg]) {
                    const uint2 rc = s_edge[seg][e];
                    int64_t r = rc.x, c = rc.y;
                    if (perm) {
                        r = r < n ? perm[r] : 0;
                        c = c < n ? perm[c] : 0;
                    }
                    rows[idx] = r;
                    cols[idx] = c;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_rg_decode(const int64_t* __restrict__ slots, int64_t count, int kind, uint64_t cols,
                                                     int64_t* __restrict__ row_out, int64_t* __restrict__ col_out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        uint64_t r, c;
        rg_decode(kind, cols, (uint64_t)slots[i], r, c);
        row_out[i] = (int64_t)r;
        col_out[i] = (int64_t)c;
    }
}

__global__ __launch_bounds__(kBlock) void k_rg_draws(uint64_t N, uint32_t k0, uint32_t k1, uint32_t tag, uint64_t round, int64_t first, int64_t count,
                                                    int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock)
        out[i] = (int64_t)rg_below(N, k0, k1, tag, round, (uint64_t)(first + i));
}

// G(n,m): sorted (value, draw index) pairs -> first_by_draw[draw] = 1 where the draw is the first occurrence of its value
__global__ __launch_bounds__(kBlock) void k_rg_first(const int64_t* __restrict__ value, const int32_t* __restrict__ draw, int64_t count,
                                                    int32_t* __restrict__ first_by_draw) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        const int64_t d = draw[i];
        if ((uint64_t)d < (uint64_t)count) first_by_draw[d] = i == 0 || value[i] != value[i - 1];
    }
}

// keep[i] = the sorted entry i is a first occurrence and fewer than m first occurrences have a smaller draw index (rank: the scan of first_by_draw)
__global__ __launch_bounds__(kBlock) void k_rg_keep(const int64_t* __restrict__ value, const int32_t* __restrict__ draw, const int64_t* __restrict__ rank,
                                                   int64_t count, int64_t m, int32_t* __restrict__ keep) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        const int64_t d = draw[i];
        const bool first = i == 0 || value[i] != value[i - 1];
        keep[i] = first && (uint64_t)d < (uint64_t)count && rank[d] < m;
    }
}

__global__ __launch_bounds__(kBlock) void k_rg_compact(const int64_t* __restrict__ value, const int64_t* __restrict__ pos, int64_t count, int64_t cap,
                                                      int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        const int64_t p = pos[i];
        if (pos[i + 1] > p && p >= 0 && p < cap) out[p] = value[i];
    }
}

// the slots of [0, N) that are not in the ascending, distinct list ex[0 .. k): out[o] = o + #{j : ex[j] - j <= o}
__global__ __launch_bounds__(kBlock) void k_rg_complement(const int64_t* __restrict__ ex, int64_t k, int64_t count, int64_t* __restrict__ out) {
    for (int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x; o < count; o += (int64_t)gridDim.x * kBlock) {
        int64_t lo = 0, hi = k;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (ex[mid] - mid <= o) lo = mid + 1; else hi = mid;
        }
        out[o] = o + lo;
    }
}

__global__ __launch_bounds__(kBlock) void k_rg_keys(const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t count, int64_t n,
                                                   int64_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) keys[i] = row[i] * n + col[i];
}

// Watts-Strogatz: edge e = (k - 1) n + v is v -> (v + k) mod n; rewired to a uniform target when its decision draw is below thr
__global__ __launch_bounds__(kBlock) void k_ws_edges(int64_t n, int64_t count, uint32_t k0, uint32_t k1, uint64_t thr, int always, int undirected,
                                                    int64_t* __restrict__ row, int64_t* __restrict__ col) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += (int64_t)gridDim.x * kBlock) {
        const int64_t v = e % n, k = e / n + 1;
        int64_t u = v, w = (v + k) % n;
        if (always || rg_word(k0, k1, PP_RG_TAG_WS_DECIDE, 0, (uint64_t)e) < thr) w = (int64_t)rg_below((uint64_t)n, k0, k1, PP_RG_TAG_WS_TARGET, 0, (uint64_t)e);
        if (undirected && u > w) { const int64_t x = u; u = w; w = x; }
        row[e] = u;
        col[e] = w;
    }
}

// sorted (key, edge) pairs, key = row n + col: flag[edge] = the edge is a surplus copy of its key (not the copy of smallest index) or a loop
__global__ __launch_bounds__(kBlock) void k_ws_offenders(const int64_t* __restrict__ key, const int32_t* __restrict__ edge, int64_t count, int64_t n,
                                                        int dups, int loops, int32_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        const int64_t kk = key[i], d = edge[i];
        const bool bad = (dups && i > 0 && key[i - 1] == kk) || (loops && kk / n == kk % n);
        if ((uint64_t)d < (uint64_t)count) flag[d] = bad;
    }
}

__global__ __launch_bounds__(kBlock) void k_ws_redraw(int64_t n, int64_t count, uint32_t k0, uint32_t k1, uint64_t round, int undirected,
                                                     const int32_t* __restrict__ flag, int64_t* __restrict__ row, int64_t* __restrict__ col) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += (int64_t)gridDim.x * kBlock) {
        if (!flag[e]) continue;
        // odd rounds keep the first end, even rounds the second: an edge whose kept end has no free partner left is not stuck with it
        int64_t u = (round & 1) ? row[e] : col[e], w = (int64_t)rg_below((uint64_t)n, k0, k1, PP_RG_TAG_WS_REPAIR, round, (uint64_t)e);
        if (undirected && u > w) { const int64_t x = u; u = w; w = x; }
        row[e] = u;
        col[e] = w;
    }
}

// ---- degree-sequence models (Molloy-Reed): DESIGN.md "Degree-sequence models" has the rules, tests/cpu_ops_degree_models.py restates them
constexpr uint32_t kMrNone = 0xFFFFFFFFu;      // claim[f]: no offender drew f

// stub s belongs to the node v with ptr[v] <= s < ptr[v + 1] (ptr[0] == 0, ptr[n] == stubs; a node of degree 0 owns no stub)
__global__ __launch_bounds__(kBlock) void k_mr_stubs(const int64_t* __restrict__ ptr, int64_t n, int64_t stubs, uint32_t k0, uint32_t k1,
                                                    int32_t* __restrict__ node, int64_t* __restrict__ key) {
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < stubs; s += (int64_t)gridDim.x * kBlock) {
        int64_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (ptr[mid] <= s) lo = mid; else hi = mid;
        }
        node[s] = (int32_t)lo;
        key[s] = (int64_t)rg_word(k0, k1, PP_RG_TAG_MR_SHUFFLE, 0, (uint64_t)s);
    }
}

// edge i joins the stubs at the sorted positions 2 i and 2 i + 1, ends sorted
__global__ __launch_bounds__(kBlock) void k_mr_pair(const int32_t* __restrict__ node, const int32_t* __restrict__ order, int64_t edges, int64_t n,
                                                   int64_t* __restrict__ row, int64_t* __restrict__ col) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < edges; i += (int64_t)gridDim.x * kBlock) {
        const int64_t s0 = order[2 * i], s1 = order[2 * i + 1];
        int64_t u = (uint64_t)s0 < (uint64_t)(2 * edges) ? node[s0] : 0, w = (uint64_t)s1 < (uint64_t)(2 * edges) ? node[s1] : 0;
        if ((uint64_t)u >= (uint64_t)n) u = 0;                                          // (an edge never names a node that is not there)
        if ((uint64_t)w >= (uint64_t)n) w = 0;
        row[i] = u < w ? u : w;
        col[i] = u < w ? w : u;
    }
}

// claim[f] = the smallest offender whose victim draw is f (a minimum: the order of the atomics does not matter)
__global__ __launch_bounds__(kBlock) void k_mr_claim(const int32_t* __restrict__ flag, int64_t edges, uint32_t k0, uint32_t k1, uint64_t round,
                                                    uint32_t* __restrict__ claim) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < edges; e += (int64_t)gridDim.x * kBlock) {
        if (!flag[e]) continue;
        const uint64_t f = rg_below((uint64_t)edges, k0, k1, PP_RG_TAG_MR_VICTIM, round, (uint64_t)e);            // (a multiply-high: f < edges)
        atomicMin(&claim[f], (uint32_t)e);
    }
}

__device__ __forceinline__ bool mr_present(const int64_t* __restrict__ sorted_key, int64_t count, int64_t key) {
    int64_t lo = 0, hi = count;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < count && sorted_key[lo] == key;
}

// An offender e acts iff its victim f is another edge, f is claimed by e and nobody drew e: acting pairs are disjoint (an acting offender is
// nobody's victim, its victim is its own and does not act), so both edges are read and written with plain accesses.  sorted_key and flag are
// the round-start snapshot; nothing here reads an edge another lane may write.
__global__ __launch_bounds__(kBlock) void k_mr_swap(const int32_t* __restrict__ flag, const uint32_t* __restrict__ claim,
                                                   const int64_t* __restrict__ sorted_key, int64_t edges, int64_t n, uint32_t k0, uint32_t k1,
                                                   uint64_t round, int multi, int64_t* __restrict__ row, int64_t* __restrict__ col) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < edges; e += (int64_t)gridDim.x * kBlock) {
        if (!flag[e]) continue;
        const int64_t f = (int64_t)rg_below((uint64_t)edges, k0, k1, PP_RG_TAG_MR_VICTIM, round, (uint64_t)e);   // the draw of k_mr_claim again
        if (f == e || claim[f] != (uint32_t)e || claim[e] != kMrNone) continue;
        const int64_t a = row[e], b = col[e];
        int64_t c = row[f], d = col[f];
        if (rg_word(k0, k1, PP_RG_TAG_MR_SIDE, round << 32, (uint64_t)e) & 1) { const int64_t x = c; c = d; d = x; }
        const int64_t e0 = a < c ? a : c, e1 = a < c ? c : a, f0 = b < d ? b : d, f1 = b < d ? d : b;
        const bool bad_e = e0 == e1 || (!multi && mr_present(sorted_key, edges, e0 * n + e1));
        const bool bad_f = f0 == f1 || (!multi && (mr_present(sorted_key, edges, f0 * n + f1) || (f0 == e0 && f1 == e1)));
        if ((int)bad_e + (int)bad_f > 1 + (flag[f] != 0)) continue;                    // worse than before: the proposal is dropped
        row[e] = e0; col[e] = e1;
        row[f] = f0; col[f] = f1;
    }
}

// Erdös-Gallai, one lane per r = 1 .. n: asc holds the degrees ascending (all in 0 .. n - 1), scan its exclusive scan, so the descending
// sequence is d_i = asc[n - i] and P_r = scan[n] - scan[n - r].  With c = max(r, #{i : d_i > r}) the condition is
// P_r <= r (r - 1) + r (c - r) + P_n - P_c; every term stays below 2^62.  Every violating lane stores the same 1.
__global__ __launch_bounds__(kBlock) void k_eg_check(const int64_t* __restrict__ asc, const int64_t* __restrict__ scan, int64_t n,
                                                    int32_t* __restrict__ violated) {
    const int64_t total = scan[n];
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x + 1; r <= n; r += (int64_t)gridDim.x * kBlock) {
        int64_t lo = 0, hi = n;                                                         // the first position of asc with a degree > r
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (asc[mid] <= r) lo = mid + 1; else hi = mid;
        }
        const int64_t above = n - lo, c = above > r ? above : r;
        const int64_t lhs = total - scan[n - r], rhs = r * (r - 1) + r * (c - r) + scan[n - c];
        if (lhs > rhs || (r == 1 && (total & 1))) violated[0] = 1;
    }
}

static unsigned rg_grid(int64_t items) {
    int64_t g = ceil_div(items > 0 ? items : 1, kBlock);
    const int64_t share = shared_grid(kMaxGrid);
    if (g > share) g = share;
    note_persistent_grid(g);
    return (unsigned)g;
}

}  // namespace pp

extern "C" {

int pp_rg_region_count(const int64_t* regions, int64_t n_regions, int64_t n_chunks, int64_t seed, int64_t* counts, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n_regions >= 1 && n_regions < (1 << 30) && n_chunks >= 0, PP_ERR_ARG, "pp_rg_region_count: bad sizes");
    PP_REQUIRE(regions && (n_chunks == 0 || counts), PP_ERR_ARG, "pp_rg_region_count: null pointer");
    if (n_chunks == 0) return PP_OK;
    k_rg_count<<<rg_grid(n_chunks), kBlock, 0, (hipStream_t)stream>>>(regions, (int)n_regions, n_chunks, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32),
                                                                       PP_RG_TAG_REGION, counts);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_region_fill(const int64_t* regions, int64_t n_regions, int64_t n_chunks, int64_t seed, const int64_t* offsets, const int64_t* perm,
                      int64_t n, int64_t total, int64_t* rows, int64_t* cols, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n_regions >= 1 && n_regions < (1 << 30) && n_chunks >= 0 && total >= 0, PP_ERR_ARG, "pp_rg_region_fill: bad sizes");
    PP_REQUIRE(n >= 0 && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_rg_region_fill: 2^31 - 1 nodes or more");
    PP_REQUIRE(regions && (n_chunks == 0 || offsets) && (total == 0 || (rows && cols)), PP_ERR_ARG, "pp_rg_region_fill: null pointer");
    if (n_chunks == 0 || total == 0) return PP_OK;
    k_rg_fill<<<rg_grid(n_chunks), kBlock, 0, (hipStream_t)stream>>>(regions, (int)n_regions, n_chunks, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32),
                                                                      PP_RG_TAG_REGION, offsets, perm, n, total, rows, cols);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_decode(const int64_t* slots, int64_t count, int kind, int64_t cols, int64_t* rows_out, int64_t* cols_out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && kind >= 0 && kind <= 3 && cols >= 0, PP_ERR_ARG, "pp_rg_decode: bad arguments");
    PP_REQUIRE(count == 0 || (slots && rows_out && cols_out), PP_ERR_ARG, "pp_rg_decode: null pointer");
    if (count == 0) return PP_OK;
    k_rg_decode<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(slots, count, kind, (uint64_t)cols, rows_out, cols_out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_draws(int64_t below, int64_t seed, int tag, int64_t round, int64_t first, int64_t count, int64_t* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(below != 0 && count >= 0 && first >= 0 && tag >= 0 && tag < 256 && round >= 0 && round < (1 << 24), PP_ERR_ARG, "pp_rg_draws: bad arguments");
    PP_REQUIRE(count == 0 || out, PP_ERR_ARG, "pp_rg_draws: null pointer");
    if (count == 0) return PP_OK;
    k_rg_draws<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>((uint64_t)below, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)tag,
                                                                  (uint64_t)round, first, count, out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_first(const int64_t* value, const int32_t* draw, int64_t count, int32_t* first_by_draw, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && (count == 0 || (value && draw && first_by_draw)), PP_ERR_ARG, "pp_rg_first: bad arguments");
    if (count == 0) return PP_OK;
    k_rg_first<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(value, draw, count, first_by_draw);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_keep(const int64_t* value, const int32_t* draw, const int64_t* rank, int64_t count, int64_t m, int32_t* keep, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && (count == 0 || (value && draw && rank && keep)), PP_ERR_ARG, "pp_rg_keep: bad arguments");
    if (count == 0) return PP_OK;
    k_rg_keep<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(value, draw, rank, count, m, keep);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_compact(const int64_t* value, const int64_t* pos, int64_t count, int64_t cap, int64_t* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && cap >= 0 && (count == 0 || (value && pos)) && (cap == 0 || out), PP_ERR_ARG, "pp_rg_compact: bad arguments");
    if (count == 0 || cap == 0) return PP_OK;
    k_rg_compact<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(value, pos, count, cap, out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_complement(const int64_t* excluded, int64_t k, int64_t count, int64_t* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(k >= 0 && count >= 0 && (k == 0 || excluded) && (count == 0 || out), PP_ERR_ARG, "pp_rg_complement: bad arguments");
    if (count == 0) return PP_OK;
    k_rg_complement<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(excluded, k, count, out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_keys(const int64_t* rows, const int64_t* cols, int64_t count, int64_t n, int64_t* keys, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && n >= 0 && n < (int64_t)0x7fffffff && (count == 0 || (rows && cols && keys)), PP_ERR_ARG, "pp_rg_keys: bad arguments");
    if (count == 0) return PP_OK;
    k_rg_keys<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(rows, cols, count, n, keys);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_ws_edges(int64_t n, int64_t s, int64_t seed, int64_t threshold, int always, int undirected, int64_t* rows, int64_t* cols, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 1 && s >= 0 && n < (int64_t)0x7fffffff && s < (int64_t)0x7fffffff, PP_ERR_ARG, "pp_rg_ws_edges: bad sizes");
    const int64_t count = n * s;
    PP_REQUIRE(count == 0 || (rows && cols), PP_ERR_ARG, "pp_rg_ws_edges: null pointer");
    if (count == 0) return PP_OK;
    k_ws_edges<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(n, count, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint64_t)threshold, always,
                                                                  undirected, rows, cols);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_ws_offenders(const int64_t* key, const int32_t* edge, int64_t count, int64_t n, int dups, int loops, int32_t* flag, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && n >= 1 && (count == 0 || (key && edge && flag)), PP_ERR_ARG, "pp_rg_ws_offenders: bad arguments");
    if (count == 0) return PP_OK;
    k_ws_offenders<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(key, edge, count, n, dups, loops, flag);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_ws_redraw(int64_t n, int64_t count, int64_t seed, int64_t round, int undirected, const int32_t* flag, int64_t* rows, int64_t* cols,
                    pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(count >= 0 && n >= 1 && round >= 0 && round < (1 << 24) && (count == 0 || (flag && rows && cols)), PP_ERR_ARG, "pp_rg_ws_redraw: bad arguments");
    if (count == 0) return PP_OK;
    k_ws_redraw<<<rg_grid(count), kBlock, 0, (hipStream_t)stream>>>(n, count, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint64_t)round, undirected, flag,
                                                                   rows, cols);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_mr_stubs(const int64_t* ptr, int64_t n, int64_t stubs, int64_t seed, int32_t* node, int64_t* key, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && stubs >= 0, PP_ERR_ARG, "pp_rg_mr_stubs: bad sizes");
    PP_REQUIRE(n < (int64_t)0x7fffffff && stubs < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_rg_mr_stubs: 2^31 - 1 nodes or stubs, or more");
    PP_REQUIRE(stubs == 0 || (n >= 1 && ptr && node && key), PP_ERR_ARG, "pp_rg_mr_stubs: null pointer, or stubs without nodes");
    if (stubs == 0) return PP_OK;
    k_mr_stubs<<<rg_grid(stubs), kBlock, 0, (hipStream_t)stream>>>(ptr, n, stubs, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), node, key);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_mr_pair(const int32_t* node, const int32_t* order, int64_t edges, int64_t n, int64_t* rows, int64_t* cols, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(edges >= 0 && n >= 0, PP_ERR_ARG, "pp_rg_mr_pair: bad sizes");
    PP_REQUIRE(n < (int64_t)0x7fffffff && 2 * edges < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_rg_mr_pair: 2^31 - 1 nodes or stubs, or more");
    PP_REQUIRE(edges == 0 || (n >= 1 && node && order && rows && cols), PP_ERR_ARG, "pp_rg_mr_pair: null pointer, or edges without nodes");
    if (edges == 0) return PP_OK;
    k_mr_pair<<<rg_grid(edges), kBlock, 0, (hipStream_t)stream>>>(node, order, edges, n, rows, cols);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_mr_claim(const int32_t* flag, int64_t edges, int64_t seed, int64_t round, uint32_t* claim, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(edges >= 0 && round >= 0 && round < (1 << 24) && (edges == 0 || (flag && claim)), PP_ERR_ARG, "pp_rg_mr_claim: bad arguments");
    PP_REQUIRE(edges < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_rg_mr_claim: 2^31 - 1 edges or more");
    if (edges == 0) return PP_OK;
    PP_HIP(hipMemsetAsync(claim, 0xFF, (size_t)edges * sizeof(uint32_t), (hipStream_t)stream));                      // kMrNone in every word
    k_mr_claim<<<rg_grid(edges), kBlock, 0, (hipStream_t)stream>>>(flag, edges, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint64_t)round, claim);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_mr_swap(const int32_t* flag, const uint32_t* claim, const int64_t* sorted_key, int64_t edges, int64_t n, int64_t seed, int64_t round,
                  int multi, int64_t* rows, int64_t* cols, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(edges >= 0 && n >= 1 && round >= 0 && round < (1 << 24), PP_ERR_ARG, "pp_rg_mr_swap: bad arguments");
    PP_REQUIRE(n < (int64_t)0x7fffffff && edges < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_rg_mr_swap: 2^31 - 1 nodes or edges, or more");
    PP_REQUIRE(edges == 0 || (flag && claim && sorted_key && rows && cols), PP_ERR_ARG, "pp_rg_mr_swap: null pointer");
    if (edges == 0) return PP_OK;
    k_mr_swap<<<rg_grid(edges), kBlock, 0, (hipStream_t)stream>>>(flag, claim, sorted_key, edges, n, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32),
                                                                 (uint64_t)round, multi, rows, cols);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_rg_eg_check(const int64_t* asc, const int64_t* scan, int64_t n, int32_t* violated, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && violated && (n == 0 || (asc && scan)), PP_ERR_ARG, "pp_rg_eg_check: bad arguments");
    PP_REQUIRE(n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_rg_eg_check: 2^31 - 1 degrees or more");
    PP_HIP(hipMemsetAsync(violated, 0, sizeof(int32_t), (hipStream_t)stream));
    if (n == 0) return PP_OK;
    k_eg_check<<<rg_grid(n), kBlock, 0, (hipStream_t)stream>>>(asc, scan, n, violated);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
