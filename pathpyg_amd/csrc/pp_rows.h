// pathpyg_amd — the row work split and the fixed-shape folds shared by the kernels that walk neighbour lists (pp_graph_triads.hip,
// pp_graph_wl.hip, pp_graph_power.hip, pp_graph_layout.hip).
//
// The split: a row (a node's list, a pair of lists) belongs to a GROUP of `width` lanes, a power of two from 1 to a wave; lane j takes the
// entries j, j + width, ... in order and the lanes fold by a butterfly (group_sum).  A row of heavy_min entries or more is left to a second
// launch with a whole workgroup per row: thread j takes the entries j, j + 256, ... and the workgroup folds (block_sum_fixed).  Sums over
// the rows are one partial per workgroup, folded by index (fold_parts).  Every fold has one shape, so the bits of a float64 sum depend on
// the list lengths, `width` and heavy_min only, never on the grid's schedule.  The group loop itself stays in each kernel: what a lane
// carries across the butterfly differs from kernel to kernel.
#pragma once
#include "pp_common.h"

namespace pp {

constexpr int64_t kHeavyMinDefault = 1024;             // a row of this many entries or more gets a whole workgroup

// workgroups for `items` at `per_block` a workgroup, at least 1 and at most `cap`: the kernels stride over what is left
static inline unsigned capped_grid(int64_t items, int64_t per_block, int64_t cap = kMaxGrid) {
    const int64_t g = ceil_div(items > 0 ? items : 1, per_block);
    return (unsigned)(g > cap ? cap : g);
}

// lanes per row: the caller's `group`, else the smallest power of two that is no less than the mean list length, between 4 and a wave
static inline int row_width(int group, int64_t rows, int64_t entries) {
    if (group > 0) return group;
    const int64_t mean = rows > 0 ? ceil_div(entries, rows) : 1;
    int w = 4;
    while (w < kWave && w < mean) w <<= 1;
    return w;
}
static inline bool row_width_ok(int group) { return group == 0 || (group >= 1 && group <= kWave && (group & (group - 1)) == 0); }

// [lo, hi) = the entries of row v, clamped into [0, total] and never descending: a pointer is not trusted past the entry array
__device__ __forceinline__ void row_span(const int64_t* ptr, int64_t v, int64_t total, int64_t& lo, int64_t& hi) {
    int64_t p = ptr[v], q = ptr[v + 1];
    p = p < 0 ? 0 : (p > total ? total : p);
    q = q > total ? total : q;
    lo = p;
    hi = q < p ? p : q;
}

// butterfly over the `width` lanes of a group, in place, of every value a lane carries (one loop: the shuffles of the values interleave);
// every lane of the wave must be here (partners share the row)
template <typename... T>
__device__ __forceinline__ void group_sum(int width, T&... v) {
    for (int d = width >> 1; d > 0; d >>= 1) ((v += __shfl_xor(v, d, kWave)), ...);
}

// all threads of the workgroup get the sum of one double per thread in a fixed shape: wave butterfly, then the waves in order.  The waves
// are added to 0.0, not to the first wave's word: partials that are all -0.0 fold to +0.0 (pp_selection.hip's fold, which starts from the
// first wave, gives -0.0 there — the two are not interchangeable, and results written before this header existed hold these bits)
__device__ __forceinline__ double block_sum_fixed(double v, double* scratch) {
    v = wave_sum(v);
    __syncthreads();                                                                    // (scratch may still be read from the previous fold)
    if (lane_id() == 0) scratch[wave_id()] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) t += scratch[w];
    return t;
}
__device__ __forceinline__ double block_max_fixed(double v, double* scratch) {
    v = wave_max(v);
    __syncthreads();
    if (lane_id() == 0) scratch[wave_id()] = v;
    __syncthreads();
    double t = scratch[0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) t = scratch[w] > t ? scratch[w] : t;
    return t;
}

// partials part[0 .. count) folded by one workgroup in a fixed shape (thread t adds t, t + 256, ... in order, then block_sum_fixed); the
// same bits in every thread of every workgroup that asks
__device__ __forceinline__ double fold_parts(const double* part, int64_t count, double* scratch) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += kBlock) s += part[i];
    return block_sum_fixed(s, scratch);
}

// ------------------------------------------------------------------ iterations in batches
// The first words of the device state of a kernel family that iterates until a criterion holds; a family's own words follow.
enum { kDone = 0, kIters = 1, kCur = 2, kHeavyCount = 3, kStateShared = 4 };

// Enqueues up to `limit` iterations, `per_batch` at a time; after each batch the `words` state words are copied to `host` and the stream
// is synchronised once.  Stops when the device has set `done`.  `enqueue` launches one iteration and returns PP_OK or the status to pass on.
template <typename Enqueue>
static int run_batched(int64_t limit, int64_t per_batch, const int64_t* state, int64_t* host, int words, hipStream_t st, Enqueue enqueue) {
    int64_t enqueued = 0;
    while (enqueued < limit) {
        const int64_t now = limit - enqueued < per_batch ? limit - enqueued : per_batch;
        for (int64_t i = 0; i < now; ++i) {
            const int rc = enqueue();
            if (rc != PP_OK) return rc;
        }
        enqueued += now;
        PP_HIP(hipMemcpyAsync(host, state, (size_t)words * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        if (host[kDone]) break;
    }
    return PP_OK;
}

}  // namespace pp
