// pathpyg_amd — order selection of a multi-order model (reference src/pathpyG/core/multi_order_model.py:243-409) without line-graph lifts:
//   pp_walk_counts_i64      walks of length 1..K of a topology and the rows that start one (get_mon_dof, :283-309): one int64 vector pushed
//                           K times through the CSR, saturating at INT64_MAX;
//   pp_mon_layer_llh_f64    the top term  sum_e w_e log(w_e / S_row(e))  (:394-397) and the intermediate term  sum_s f_s log(1 / d(row(sel_s)))
//                           (:338-369) of one layer, straight from its CSR;
//   pp_mon_zeroth_llh_f64   the two zeroth-order terms of a walk store (:311-336, :402-407).
// The likelihood terms are float64 from the first operation on and PURE FUNCTIONS OF THE INPUT VALUES: every sum has a shape that only the
// sizes fix — a row by 64 (or, above kLongRow entries, 256) strided lanes and a butterfly, a vector by chunks of kChunk entries whose partial
// sums one final workgroup adds in index order — so neither the grid, the integer width of the row pointers nor the order in which workgroups
// finish reaches the result.  No floating-point atomics.
#include <math.h>

#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {
namespace {

constexpr int kLongRow = 1024;           // rows with more entries are walked by a whole workgroup (hubs), the others by one wave
constexpr int kChunk = 2048;             // entries per partial sum of a vector reduction: kBlock threads x 8 strided entries
constexpr int64_t kI64Max = INT64_MAX;

enum : int64_t { kBadIndex = 1, kBadPtr = 2, kMissingId = 4, kBadWalks = 8 };

__device__ __forceinline__ int64_t load_idx(const void* p, int64_t i, int wide) {
    return wide ? ((const int64_t*)p)[i] : (int64_t)((const int32_t*)p)[i];
}

// whether a pointer array starts at 0 and ends at the entry count (with ascending rows, row_bounds: every entry belongs to exactly one row)
__device__ __forceinline__ bool ptr_ends_ok(const void* ptr, int wide, int64_t n_rows, int64_t total) {
    return load_idx(ptr, 0, wide) == 0 && load_idx(ptr, n_rows, wide) == total;
}

// entries [lo, hi) of row r, clamped into [0, total): a malformed pointer array cannot send a read out of bounds (it sets kBadPtr)
__device__ __forceinline__ bool row_bounds(const void* ptr, int wide, int64_t r, int64_t total, int64_t& lo, int64_t& hi) {
    const int64_t a = load_idx(ptr, r, wide), b = load_idx(ptr, r + 1, wide);
    lo = a < 0 ? 0 : (a > total ? total : a);
    hi = b < lo ? lo : (b > total ? total : b);
    return lo == a && hi == b;
}

__device__ __forceinline__ int64_t sat_add(int64_t a, int64_t b, bool& sat) {       // a, b >= 0
    const uint64_t s = (uint64_t)a + (uint64_t)b;
    if (s > (uint64_t)kI64Max) { sat = true; return kI64Max; }
    return (int64_t)s;
}

__device__ __forceinline__ int64_t wave_sat_sum(int64_t v, bool& sat) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v = sat_add(v, __shfl_xor(v, d, kWave), sat);
    return v;
}

// the workgroup's sum of one double per thread in a fixed shape: butterfly inside each wave, then the four waves left to right, starting
// from the first wave's word (pp_rows.h's block_sum_fixed starts from 0.0 and so differs on four partials of -0.0: keep them apart)
__device__ __forceinline__ double block_sum_ltr(double v, double* s4) {
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) s4[wave_id()] = v;
    __syncthreads();
    return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// ------------------------------------------------------------------ walk counts
// The counts of one order: c[v] per node, written by the row kernels; their sum and the number of non-zero ones come from k_walk_reduce.
// A sum of up to 2^31 values below 2^63 is kept as two 64-bit words — the sum of the low and of the high 32-bit halves — so that plain integer
// atomics (one per workgroup and word) add it exactly in any order; k_walk_finish folds the words and saturates.
// order 1: c[v] = out-degree; the rows longer than kLongRow are listed once for all K steps
__global__ __launch_bounds__(kBlock) void k_walk_first(const void* ptr, int pw, int64_t n, int64_t total, int64_t* c, int32_t* long_rows,
                                                       int32_t* long_count, int32_t long_max, int64_t* status) {
    bool bad = blockIdx.x == 0 && threadIdx.x == 0 && !ptr_ends_ok(ptr, pw, n, total);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        int64_t lo, hi;
        bad |= !row_bounds(ptr, pw, r, total, lo, hi);
        c[r] = hi - lo;
        if (hi - lo > kLongRow) {
            const int32_t slot = atomicAdd(long_count, 1);
            if (slot < long_max) long_rows[slot] = (int32_t)r; else bad = true;      // (only overlapping rows of a malformed pointer array get here)
        }
    }
    if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadPtr);
}

// every column id lies in [0, n): checked once, whatever K (order 1 reads no column)
__global__ __launch_bounds__(kBlock) void k_walk_check_cols(const void* col, int cw, int64_t n_edges, int64_t n, int64_t* status) {
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        const int64_t u = load_idx(col, e, cw);
        bad |= u < 0 || u >= n;
    }
    if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadIndex);
}

// one step: next[v] = sum over the successors u of v of prev[u]; one wave per row of at most kLongRow entries
__global__ __launch_bounds__(kBlock) void k_walk_step(const void* ptr, int pw, const void* col, int cw, int64_t n, int64_t total,
                                                      const int64_t* __restrict__ prev, int64_t* __restrict__ next, int64_t* sat_flag, int64_t* status) {
    const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock;
    bool sat = false, bad = false;
    for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave_id(); r < n; r += waves) {
        int64_t lo, hi;
        row_bounds(ptr, pw, r, total, lo, hi);
        if (hi - lo > kLongRow) continue;
        int64_t c = 0;
        for (int64_t e = lo + lane_id(); e < hi; e += kWave) {
            const int64_t u = load_idx(col, e, cw);
            if (u < 0 || u >= n) { bad = true; continue; }
            c = sat_add(c, prev[u], sat);
        }
        c = wave_sat_sum(c, sat);
        if (lane_id() == 0) next[r] = c;
    }
    if (sat) atomicExch((unsigned long long*)sat_flag, 1ull);
    if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadIndex);
}

// the listed long rows: one workgroup per row
__global__ __launch_bounds__(kBlock) void k_walk_step_long(const void* ptr, int pw, const void* col, int cw, int64_t n, int64_t total,
                                                           const int64_t* __restrict__ prev, int64_t* __restrict__ next,
                                                           const int32_t* __restrict__ long_rows, const int32_t* __restrict__ long_count, int32_t long_max,
                                                           int64_t* sat_flag, int64_t* status) {
    __shared__ int64_t s_c[kWavesPerBlock];
    const int count = *long_count < long_max ? *long_count : long_max;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const int64_t r = long_rows[i];
        int64_t lo, hi;
        row_bounds(ptr, pw, r, total, lo, hi);
        int64_t c = 0;
        bool sat = false, bad = false;
        for (int64_t e = lo + threadIdx.x; e < hi; e += kBlock) {
            const int64_t u = load_idx(col, e, cw);
            if (u < 0 || u >= n) { bad = true; continue; }
            c = sat_add(c, prev[u], sat);
        }
        c = wave_sat_sum(c, sat);
        __syncthreads();
        if (lane_id() == 0) s_c[wave_id()] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t all = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) all = sat_add(all, s_c[w], sat);
            next[r] = all;
        }
        if (sat) atomicExch((unsigned long long*)sat_flag, 1ull);
        if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadIndex);
    }
}

// sum (as low / high halves) and number of non-zero entries of c[n]: per-thread partial sums, one integer atomic per workgroup and word
__global__ __launch_bounds__(kBlock) void k_walk_reduce(const int64_t* __restrict__ c, int64_t n, unsigned long long* acc_lo, unsigned long long* acc_hi,
                                                        int64_t* starts) {
    __shared__ unsigned long long s_lo[kWavesPerBlock], s_hi[kWavesPerBlock], s_nz[kWavesPerBlock];
    unsigned long long lo = 0, hi = 0, nz = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint64_t v = (uint64_t)c[i];
        lo += v & 0xffffffffull;
        hi += v >> 32;
        nz += v != 0;
    }
    lo = wave_sum(lo);
    hi = wave_sum(hi);
    nz = wave_sum(nz);
    if (lane_id() == 0) { s_lo[wave_id()] = lo; s_hi[wave_id()] = hi; s_nz[wave_id()] = nz; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) { lo += s_lo[w]; hi += s_hi[w]; nz += s_nz[w]; }
        if (lo) atomicAdd(acc_lo, lo);
        if (hi) atomicAdd(acc_hi, hi);
        if (nz) atomicAdd((unsigned long long*)starts, nz);
    }
}

// totals[k] = min(hi * 2^32 + lo, INT64_MAX); a total beyond int64 sets the order's saturation flag
__global__ void k_walk_finish(const unsigned long long* acc_lo, const unsigned long long* acc_hi, int64_t K, int64_t* totals, int64_t* sat_flags) {
    for (int64_t k = threadIdx.x; k < K; k += blockDim.x) {
        const unsigned long long lo = acc_lo[k], hi = acc_hi[k];
        unsigned long long t = (hi << 32) + lo;              // (lo < 2^63: below 2^31 halves of 32 bits; no wrap when hi < 2^31)
        bool sat = (hi >> 31) != 0 || t > (unsigned long long)kI64Max;
        totals[k] = sat ? kI64Max : (int64_t)t;
        if (sat) sat_flags[k] = 1;
    }
}

// ------------------------------------------------------------------ row sums and row terms of a weighted CSR
// kTerms == false: row_out[r] = S_r = float64 sum of the row's weights;  true: row_out[r] = sum_e w_e log(w_e / S_r)
template <bool kTerms>
__global__ __launch_bounds__(kBlock) void k_rows(const void* ptr, int pw, int64_t n_rows, int64_t total, const float* __restrict__ w,
                                                 double* __restrict__ row_out, int32_t* long_rows, int32_t* long_count, int32_t long_max,
                                                 int64_t* status) {
    const int64_t waves = (int64_t)gridDim.x * kWavesPerBlock;
    bool bad = blockIdx.x == 0 && threadIdx.x == 0 && !ptr_ends_ok(ptr, pw, n_rows, total);
    for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave_id(); r < n_rows; r += waves) {
        int64_t lo, hi;
        bad |= !row_bounds(ptr, pw, r, total, lo, hi);
        if (hi - lo > kLongRow) {
            if (lane_id() == 0) {
                const int32_t slot = atomicAdd(long_count, 1);
                if (slot < long_max) long_rows[slot] = (int32_t)r; else bad = true;      // (only overlapping rows of a malformed pointer array get here)
            }
            continue;
        }
        double s = 0.0;
        for (int64_t e = lo + lane_id(); e < hi; e += kWave) s += (double)w[e];
        s = wave_sum(s);
        if (kTerms) {
            double t = 0.0;
            for (int64_t e = lo + lane_id(); e < hi; e += kWave) {
                const double x = (double)w[e];
                t += x * log(x / s);
            }
            s = wave_sum(t);
        }
        if (lane_id() == 0) row_out[r] = s;
    }
    if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadPtr);
}

template <bool kTerms>
__global__ __launch_bounds__(kBlock) void k_rows_long(const void* ptr, int pw, int64_t total, const float* __restrict__ w, double* __restrict__ row_out,
                                                      const int32_t* __restrict__ long_rows, const int32_t* __restrict__ long_count, int32_t long_max) {
    __shared__ double s4[kWavesPerBlock];
    const int count = *long_count < long_max ? *long_count : long_max;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const int64_t r = long_rows[i];
        int64_t lo, hi;
        row_bounds(ptr, pw, r, total, lo, hi);
        double s = 0.0;
        for (int64_t e = lo + threadIdx.x; e < hi; e += kBlock) s += (double)w[e];
        s = block_sum_ltr(s, s4);
        if (kTerms) {
            double t = 0.0;
            for (int64_t e = lo + threadIdx.x; e < hi; e += kBlock) {
                const double x = (double)w[e];
                t += x * log(x / s);
            }
            s = block_sum_ltr(t, s4);
        }
        if (threadIdx.x == 0) row_out[r] = s;
    }
}

// ------------------------------------------------------------------ vector reductions in a fixed shape
// What entry i of the vector is: one functor per term.
struct VecPlain {            // v[i]
    const double* v;
    __device__ double operator()(int64_t i, int64_t&) const { return v[i]; }
};

struct VecEntropy {          // C_i log(C_i / sum C): zeroth-order model, multi_order_model.py:402-407
    const double *c, *sum;
    __device__ double operator()(int64_t i, int64_t&) const { return c[i] * log(c[i] / *sum); }
};

struct VecIntermediate {     // f_s log(1 / d(row of edge sel_s)), d the UNWEIGHTED out-degree (transition_probabilities() without edge_attr, :363)
    const void* ptr;
    int pw;
    int64_t n_rows, total;
    const void* sel;
    int sw;
    const float* freq;
    __device__ double operator()(int64_t i, int64_t& status) const {
        const int64_t e = load_idx(sel, i, sw);
        if (e < 0 || e >= total) { status |= kBadIndex; return 0.0; }
        int64_t lo = 0, hi = n_rows + 1;                     // first index whose pointer exceeds e; the row is the one before it
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (load_idx(ptr, mid, pw) > e) hi = mid; else lo = mid + 1;
        }
        const int64_t r = lo - 1;
        if (r < 0 || r >= n_rows) { status |= kBadPtr; return 0.0; }
        const int64_t d = load_idx(ptr, r + 1, pw) - load_idx(ptr, r, pw);
        return (double)freq[i] * log(1.0 / (double)d);
    }
};

struct VecStart {            // f_w log(c[first node of walk w] / P): :325-336
    const int64_t *seq, *offs;
    const int32_t* nptr;
    const float* f;
    int64_t positions, n;
    __device__ double operator()(int64_t i, int64_t& status) const {
        const int64_t p = offs[i];
        if (p < 0 || p >= positions || offs[i + 1] <= p) { status |= kBadWalks; return 0.0; }
        const int64_t v = seq[p];
        if (v < 0 || v >= n) { status |= kBadIndex; return 0.0; }
        const double c = (double)(nptr[v + 1] - nptr[v]);
        return (double)f[i] * log(c / (double)positions);
    }
};

// partial[c] = entries [c * kChunk, (c + 1) * kChunk): thread t adds its 8 strided entries in ascending order, then block_sum_ltr
template <typename F>
__global__ __launch_bounds__(kBlock) void k_chunks(F f, int64_t n, double* __restrict__ partial, int64_t* status) {
    __shared__ double s4[kWavesPerBlock];
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    int64_t st = 0;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kChunk / kBlock; ++j) {
            const int64_t i = c * kChunk + (int64_t)j * kBlock + threadIdx.x;
            if (i < n) acc += f(i, st);
        }
        acc = block_sum_ltr(acc, s4);
        if (threadIdx.x == 0) partial[c] = acc;
    }
    if (st) atomicOr((unsigned long long*)status, (unsigned long long)st);
}

struct FinalJob {
    const double* partial;
    int64_t count;
    double* out;
};
struct FinalJobs {
    FinalJob job[2];
};

// one workgroup per job adds the partial sums in index order (thread t: t, t + 256, ...), then block_sum_ltr
__global__ __launch_bounds__(kBlock) void k_final(FinalJobs js) {
    __shared__ double s4[kWavesPerBlock];
    const FinalJob j = js.job[blockIdx.x];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < j.count; i += kBlock) acc += j.partial[i];
    acc = block_sum_ltr(acc, s4);
    if (threadIdx.x == 0) *j.out = acc;
}

static inline int64_t chunks_of(int64_t n) { return ceil_div(n > 0 ? n : 1, kChunk); }
static inline unsigned chunk_grid(int64_t n) {
    const int64_t c = chunks_of(n);
    return (unsigned)(c > kMaxGrid ? kMaxGrid : c);
}
static inline int64_t long_cap(int64_t entries) { return entries / kLongRow + 1; }
static inline unsigned long_grid(int64_t entries) {
    const int64_t c = long_cap(entries);
    return (unsigned)(c > 1024 ? 1024 : c);
}

// ------------------------------------------------------------------ zeroth order: helpers
__global__ __launch_bounds__(kBlock) void k_zero_keys(const int64_t* __restrict__ seq, int64_t positions, int64_t n, uint32_t* __restrict__ key,
                                                      int64_t* status) {
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < positions; p += stride) {
        const int64_t v = seq[p];
        const bool ok = v >= 0 && v < n;
        bad |= !ok;
        key[p] = ok ? (uint32_t)v : 0u;
    }
    if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadIndex);
}

// nptr[v] = first sorted position whose node is >= v (v = 0..n); a node without positions sets kMissingId
__global__ __launch_bounds__(kBlock) void k_zero_node_ptr(const uint32_t* __restrict__ key_sorted, int64_t positions, int64_t n, int32_t* __restrict__ nptr,
                                                          int64_t* status) {
    bool missing = false;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v <= n; v += stride) {
        const int64_t at = lower_bound_dev<uint32_t, int64_t>(key_sorted, 0, positions, (uint32_t)v);
        nptr[v] = (int32_t)at;
        if (v < n && (at >= positions || key_sorted[at] != (uint32_t)v)) missing = true;
    }
    if (missing) atomicOr((unsigned long long*)status, (unsigned long long)kMissingId);
}

// w_sorted[i] = weight of the walk that holds position pos_sorted[i]; the walk lengths are checked on the way
__global__ __launch_bounds__(kBlock) void k_zero_weights(const uint32_t* __restrict__ pos_sorted, int64_t positions, const int64_t* __restrict__ offs,
                                                         int64_t walks, const float* __restrict__ f, float* __restrict__ w_sorted, int64_t* status) {
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    if (blockIdx.x == 0 && threadIdx.x == 0 && offs[walks] != positions) bad = true;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < positions; i += stride) {
        const int64_t p = pos_sorted[i];
        int64_t walk = upper_bound_dev<int64_t, int64_t>(offs, 0, walks + 1, p) - 1;
        if (walk < 0 || walk >= walks) { bad = true; walk = 0; }
        else if (!(offs[walk] <= p && p < offs[walk + 1])) bad = true;
        w_sorted[i] = f[walk];
    }
    if (bad) atomicOr((unsigned long long*)status, (unsigned long long)kBadWalks);
}

struct ZerothWs {
    int64_t* offs;
    void* scan_ws;
    uint32_t *key, *key_sorted, *pos_sorted;
    void* sort_ws;
    int32_t* nptr;
    float* w_sorted;
    double *row_sum, *partial, *total;
    int32_t *long_rows, *long_count;
    size_t scan_bytes, sort_bytes, bytes;
};

static ZerothWs zeroth_ws(void* ws, int64_t positions, int64_t walks, int64_t n) {
    Arena a(ws, (size_t)-1);
    ZerothWs z;
    z.scan_bytes = scan_ws_bytes(walks);
    z.sort_bytes = sort_ws_bytes(positions, 4);
    z.offs = a.take<int64_t>(walks + 1);
    z.scan_ws = a.take<char>((int64_t)z.scan_bytes);
    z.key = a.take<uint32_t>(positions);
    z.key_sorted = a.take<uint32_t>(positions);
    z.pos_sorted = a.take<uint32_t>(positions);
    z.sort_ws = a.take<char>((int64_t)z.sort_bytes);
    z.nptr = a.take<int32_t>(n + 1);
    z.w_sorted = a.take<float>(positions);
    z.row_sum = a.take<double>(n);
    z.partial = a.take<double>(chunks_of(n) + chunks_of(walks));
    z.total = a.take<double>(1);
    z.long_rows = a.take<int32_t>(long_cap(positions));
    z.long_count = a.take<int32_t>(1);
    z.bytes = a.used;
    return z;
}

struct LayerWs {
    double *row_term, *partial;
    int32_t *long_rows, *long_count;
    size_t bytes;
};

static LayerWs layer_ws(void* ws, int64_t n_rows, int64_t n_edges, int64_t n_sel) {
    Arena a(ws, (size_t)-1);
    LayerWs l;
    l.row_term = a.take<double>(n_rows);
    l.partial = a.take<double>(chunks_of(n_rows) + chunks_of(n_sel));
    l.long_rows = a.take<int32_t>(long_cap(n_edges));
    l.long_count = a.take<int32_t>(1);
    l.bytes = a.used;
    return l;
}

}  // namespace
}  // namespace pp

// =================================================================== C ABI
extern "C" {

size_t pp_walk_counts_ws_bytes(int64_t n, int64_t n_edges, int64_t K) {
    using namespace pp;
    return 2 * align_up((size_t)(n > 0 ? n : 1) * sizeof(int64_t)) + align_up((size_t)long_cap(n_edges) * sizeof(int32_t)) +
           align_up((size_t)(K > 0 ? 2 * K : 2) * sizeof(int64_t)) + 256;
}

int pp_walk_counts_i64(const void* row_ptr, int ptr_wide, const void* col, int col_wide, int64_t n, int64_t n_edges, int64_t K, int64_t* out,
                       void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n >= 0 && n_edges >= 0 && K >= 1, PP_ERR_ARG, "pp_walk_counts_i64: n=%lld, entries=%lld, K=%lld", (long long)n, (long long)n_edges, (long long)K);
    PP_REQUIRE(n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_walk_counts_i64: 2^31 or more rows");
    PP_REQUIRE(ws_bytes >= pp_walk_counts_ws_bytes(n, n_edges, K), PP_ERR_WORKSPACE, "pp_walk_counts_i64: workspace too small");
    PP_HIP(hipMemsetAsync(out, 0, (size_t)(3 * K + 1) * sizeof(int64_t), st));
    if (n == 0) return PP_OK;
    Arena a(ws, ws_bytes);
    int64_t* c[2] = {a.take<int64_t>(n), a.take<int64_t>(n)};
    int32_t* long_rows = a.take<int32_t>(long_cap(n_edges));
    unsigned long long* acc = a.take<unsigned long long>(2 * K);
    int32_t* long_count = a.take<int32_t>(1);
    PP_HIP(hipMemsetAsync(long_count, 0, sizeof(int32_t), st));
    PP_HIP(hipMemsetAsync(acc, 0, (size_t)(2 * K) * sizeof(unsigned long long), st));
    int64_t *totals = out, *starts = out + K, *sat = out + 2 * K, *status = out + 3 * K;
    int64_t g = ceil_div(n, kBlock);
    if (g > kMaxGrid) g = kMaxGrid;
    int64_t gr = ceil_div(n, (int64_t)kBlock * 16);            // k_walk_reduce: at most 256 workgroups = 768 atomics per order
    if (gr > 256) gr = 256;
    k_walk_first<<<(unsigned)g, kBlock, 0, st>>>(row_ptr, ptr_wide, n, n_edges, c[0], long_rows, long_count, (int32_t)long_cap(n_edges), status);
    PP_LAUNCH_CHECK();
    if (n_edges > 0) {
        int64_t gc = ceil_div(n_edges, (int64_t)kBlock * 4);
        if (gc > kMaxGrid) gc = kMaxGrid;
        k_walk_check_cols<<<(unsigned)gc, kBlock, 0, st>>>(col, col_wide, n_edges, n, status);
        PP_LAUNCH_CHECK();
    }
    for (int64_t k = 0; k < K; ++k) {
        int64_t* cur = c[k & 1];
        if (k > 0) {
            const int64_t* prev = c[(k - 1) & 1];
            k_walk_step<<<capped_grid(n, kWavesPerBlock), kBlock, 0, st>>>(row_ptr, ptr_wide, col, col_wide, n, n_edges, prev, cur, sat + k, status);
            PP_LAUNCH_CHECK();
            if (n_edges > kLongRow) {
                k_walk_step_long<<<long_grid(n_edges), kBlock, 0, st>>>(row_ptr, ptr_wide, col, col_wide, n, n_edges, prev, cur, long_rows, long_count,
                                                                      (int32_t)long_cap(n_edges), sat + k, status);
                PP_LAUNCH_CHECK();
            }
        }
        k_walk_reduce<<<(unsigned)gr, kBlock, 0, st>>>(cur, n, acc + k, acc + K + k, starts + k);
        PP_LAUNCH_CHECK();
    }
    k_walk_finish<<<1, kBlock, 0, st>>>(acc, acc + K, K, totals, sat);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_mon_layer_llh_ws_bytes(int64_t n_rows, int64_t n_edges, int64_t n_sel) {
    return pp::layer_ws(nullptr, n_rows, n_edges, n_sel).bytes;
}

int pp_mon_layer_llh_f64(const void* row_ptr, int ptr_wide, int64_t n_rows, const float* weight, int64_t n_edges, const void* sel, int sel_wide,
                         const float* freq, int64_t n_sel, double* out2, int64_t* status, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_rows >= 0 && n_edges >= 0 && n_sel >= 0, PP_ERR_ARG, "pp_mon_layer_llh_f64: negative size");
    PP_REQUIRE(n_rows < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_mon_layer_llh_f64: 2^31 or more rows");
    PP_REQUIRE(ws_bytes >= pp_mon_layer_llh_ws_bytes(n_rows, n_edges, n_sel), PP_ERR_WORKSPACE, "pp_mon_layer_llh_f64: workspace too small");
    const LayerWs l = layer_ws(ws, n_rows, n_edges, n_sel);
    PP_HIP(hipMemsetAsync(l.long_count, 0, sizeof(int32_t), st));
    PP_HIP(hipMemsetAsync(status, 0, sizeof(int64_t), st));
    PP_HIP(hipMemsetAsync(out2, 0, 2 * sizeof(double), st));
    FinalJobs js{};
    int jobs = 0;
    if (n_rows > 0) {
        k_rows<true><<<capped_grid(n_rows, kWavesPerBlock), kBlock, 0, st>>>(row_ptr, ptr_wide, n_rows, n_edges, weight, l.row_term, l.long_rows, l.long_count, (int32_t)long_cap(n_edges), status);
        PP_LAUNCH_CHECK();
        if (n_edges > kLongRow) {
            k_rows_long<true><<<long_grid(n_edges), kBlock, 0, st>>>(row_ptr, ptr_wide, n_edges, weight, l.row_term, l.long_rows, l.long_count, (int32_t)long_cap(n_edges));
            PP_LAUNCH_CHECK();
        }
        k_chunks<<<chunk_grid(n_rows), kBlock, 0, st>>>(VecPlain{l.row_term}, n_rows, l.partial, status);
        PP_LAUNCH_CHECK();
        js.job[jobs++] = FinalJob{l.partial, chunks_of(n_rows), out2};
    }
    if (n_sel > 0 && n_rows > 0) {
        double* partial = l.partial + chunks_of(n_rows);
        k_chunks<<<chunk_grid(n_sel), kBlock, 0, st>>>(VecIntermediate{row_ptr, ptr_wide, n_rows, n_edges, sel, sel_wide, freq}, n_sel, partial, status);
        PP_LAUNCH_CHECK();
        js.job[jobs++] = FinalJob{partial, chunks_of(n_sel), out2 + 1};
    }
    if (jobs) {
        k_final<<<(unsigned)jobs, kBlock, 0, st>>>(js);
        PP_LAUNCH_CHECK();
    }
    return PP_OK;
}

size_t pp_mon_zeroth_llh_ws_bytes(int64_t positions, int64_t walks, int64_t n) {
    return pp::zeroth_ws(nullptr, positions, walks, n).bytes;
}

int pp_mon_zeroth_llh_f64(const int64_t* node_sequence, int64_t positions, const int64_t* dag_num_nodes, const float* dag_weight, int64_t walks,
                          int64_t n, double* out2, int64_t* status, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(positions > 0 && walks > 0 && n > 0, PP_ERR_ARG, "pp_mon_zeroth_llh_f64: positions=%lld, walks=%lld, n=%lld", (long long)positions,
               (long long)walks, (long long)n);
    PP_REQUIRE(positions < (int64_t)0x7fffffff && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_mon_zeroth_llh_f64: 2^31 or more positions or nodes");
    PP_REQUIRE(ws_bytes >= pp_mon_zeroth_llh_ws_bytes(positions, walks, n), PP_ERR_WORKSPACE, "pp_mon_zeroth_llh_f64: workspace too small");
    const ZerothWs z = zeroth_ws(ws, positions, walks, n);
    PP_HIP(hipMemsetAsync(z.long_count, 0, sizeof(int32_t), st));
    PP_HIP(hipMemsetAsync(status, 0, sizeof(int64_t), st));
    PP_HIP(hipMemsetAsync(out2, 0, 2 * sizeof(double), st));
    int rc = exclusive_scan<int64_t, int64_t>(dag_num_nodes, walks, z.offs, true, nullptr, z.scan_ws, z.scan_bytes, st);
    if (rc != PP_OK) return rc;
    int64_t g = ceil_div(positions, kBlock);
    if (g > kMaxGrid) g = kMaxGrid;
    k_zero_keys<<<(unsigned)g, kBlock, 0, st>>>(node_sequence, positions, n, z.key, status);
    PP_LAUNCH_CHECK();
    // positions grouped by node, ascending inside a node (stable): the order in which a node's weights are added
    rc = sort_pairs<uint32_t>(z.key, nullptr, z.key_sorted, z.pos_sorted, positions, 0, bits_for((uint64_t)(n - 1)), z.sort_ws, z.sort_bytes, st);
    if (rc != PP_OK) return rc;
    int64_t gn = ceil_div(n + 1, kBlock);
    if (gn > kMaxGrid) gn = kMaxGrid;
    k_zero_node_ptr<<<(unsigned)gn, kBlock, 0, st>>>(z.key_sorted, positions, n, z.nptr, status);
    PP_LAUNCH_CHECK();
    k_zero_weights<<<(unsigned)g, kBlock, 0, st>>>(z.pos_sorted, positions, z.offs, walks, dag_weight, z.w_sorted, status);
    PP_LAUNCH_CHECK();
    // C_v = float64 sum of the walk weights over the positions at v, then sum C
    k_rows<false><<<capped_grid(n, kWavesPerBlock), kBlock, 0, st>>>(z.nptr, 0, n, positions, z.w_sorted, z.row_sum, z.long_rows, z.long_count, (int32_t)long_cap(positions), status);
    PP_LAUNCH_CHECK();
    if (positions > kLongRow) {
        k_rows_long<false><<<long_grid(positions), kBlock, 0, st>>>(z.nptr, 0, positions, z.w_sorted, z.row_sum, z.long_rows, z.long_count, (int32_t)long_cap(positions));
        PP_LAUNCH_CHECK();
    }
    k_chunks<<<chunk_grid(n), kBlock, 0, st>>>(VecPlain{z.row_sum}, n, z.partial, status);
    PP_LAUNCH_CHECK();
    FinalJobs sum{};
    sum.job[0] = FinalJob{z.partial, chunks_of(n), z.total};
    k_final<<<1, kBlock, 0, st>>>(sum);
    PP_LAUNCH_CHECK();
    double* partial_w = z.partial + chunks_of(n);
    k_chunks<<<chunk_grid(walks), kBlock, 0, st>>>(VecStart{node_sequence, z.offs, z.nptr, dag_weight, positions, n}, walks, partial_w, status);
    PP_LAUNCH_CHECK();
    k_chunks<<<chunk_grid(n), kBlock, 0, st>>>(VecEntropy{z.row_sum, z.total}, n, z.partial, status);
    PP_LAUNCH_CHECK();
    FinalJobs js{};
    js.job[0] = FinalJob{partial_w, chunks_of(walks), out2};
    js.job[1] = FinalJob{z.partial, chunks_of(n), out2 + 1};
    k_final<<<2, kBlock, 0, st>>>(js);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
