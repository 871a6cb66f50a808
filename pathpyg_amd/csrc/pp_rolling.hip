// pathpyg_amd — the weighted static graphs of ALL rolling time windows of a time-sorted event stream, for gfx950.
//
// Replaces, for the loop of the reference's RollingTimeWindow (src/pathpyG/algorithms/rolling_time_window.py:50-61),
//   TemporalGraph.to_static_graph(weighted=True, time_window=(t, t + size))      src/pathpyG/core/temporal_graph.py:180-203
// once per window — two masks over all m events, a compaction, a max read-back and a full radix-sort coalesce each time — by one
// pass over the stream:
//   pp_rolling_group    key = src << bits | dst per event (k_roll_keys: index range, timestamp order and NaN into a flag word), one stable
//                       radix sort of the keys over the time-sorted events -> `keys` (ascending) and `perm` (event of every position).
//                       A node pair's events are one run of positions, in time order: perm ascends inside a run.
//   pp_rolling_bounds   lo[w] / hi[w] = first event with time >= start_w / >= end_w (k_roll_bounds: two bisections per window, in the
//                       stream's own dtype).  Window w holds the events lo[w] <= e < hi[w]; both arrays are non-decreasing in w.
//   pp_rolling_count    one thread per position j, e = perm[j]: the windows that hold e are wa..wb (wa: first w with hi[w] > e, wb: last w
//                       with lo[w] <= e); a predecessor e' of the same pair lies in every one of them up to wb(e'), so position j is the
//                       HEAD of its pair in max(wa, wb(e') + 1) .. wb — their number (0 allowed) is cnt[j].  The per-window edge counts
//                       come from the same pass: +1 at the first and -1 behind the last head window into a [W + 1] difference array
//                       (k_roll_count; in LDS per workgroup while W fits), which the host sums after its one read-back.
//   pp_rolling_fill     scan of cnt, then every head (j, w) writes {w, j} in pair-major order (k_roll_fill), a stable radix sort on the
//                       ceil(log2 W) bits of w makes that window-major with (src, dst) order inside a window — coalesce's order — and
//                       k_roll_emit writes src, dst and the weight of every edge: the number of positions from j on, inside the run, whose
//                       event is < hi[w] (perm ascends: a galloping bisection from j), as float32; num_nodes[w] = max node + 1, an
//                       unsigned 32-bit word: node 2^31 - 1 gives 2^31.
// Windows may overlap (an event is head material in many) or leave gaps (cnt = 0); a range w0..w1 of windows restricts count and fill
// to a group whose edges fit a budget.  lo / hi are read at random by every thread: they are staged in LDS while the group has at most
// kRollLdsWindows windows and are left to the caches beyond that.
#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {

constexpr int kRollLdsWindows = 2048;      // lo, hi (and the difference array) of a group this small live in LDS: 3 x 8 KiB

enum : int32_t { kRollBadIndex = 1, kRollBadOrder = 2, kRollLongRun = 4 };

template <typename KeyT, typename TimeT>
__global__ __launch_bounds__(kBlock) void k_roll_keys(const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                     const TimeT* __restrict__ time, int64_t m, int64_t num_nodes, int bits,
                                                     KeyT* __restrict__ keys, int32_t* __restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
        const int64_t u = load_stream(src + i), v = load_stream(dst + i);
        const bool in_range = u >= 0 && u < num_nodes && v >= 0 && v < num_nodes;
        if (!in_range) bad |= kRollBadIndex;
        keys[i] = in_range ? (KeyT)(((uint64_t)u << bits) | (uint64_t)v) : (KeyT)0;
        const TimeT t = time[i];
        if (t != t || (i + 1 < m && descends(t, time[i + 1]))) bad |= kRollBadOrder;
    }
    if (bad) atomicOr(flags, bad);
}

template <typename TimeT>
__global__ __launch_bounds__(kBlock) void k_roll_bounds(const TimeT* __restrict__ time, int64_t m, const TimeT* __restrict__ starts,
                                                       const TimeT* __restrict__ ends, int64_t W, int32_t* __restrict__ lo,
                                                       int32_t* __restrict__ hi) {
    const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (w >= W) return;
    lo[w] = (int32_t)lower_bound_dev<TimeT, int64_t>(time, 0, m, starts[w]);
    hi[w] = (int32_t)lower_bound_dev<TimeT, int64_t>(time, 0, m, ends[w]);
}

// Windows of [w0, w1) in which position j is the head of its pair: a..b (empty when a > b).  lo / hi hold window w at index w - base.
template <typename KeyT>
__device__ __forceinline__ void head_range(const KeyT* __restrict__ keys, const uint32_t* __restrict__ perm, int64_t j,
                                           const int32_t* lo, const int32_t* hi, int base, int w0, int w1, int& a, int& b) {
    const int32_t e = (int32_t)perm[j];
    a = base + upper_bound_dev<int32_t, int>(hi, w0 - base, w1 - base, e);            // first w with hi[w] > e
    b = base + upper_bound_dev<int32_t, int>(lo, w0 - base, w1 - base, e) - 1;        // last w with lo[w] <= e
    if (j > 0 && keys[j - 1] == keys[j]) {
        const int before = base + upper_bound_dev<int32_t, int>(lo, w0 - base, w1 - base, (int32_t)perm[j - 1]);      // the predecessor's wb + 1
        a = before > a ? before : a;
    }
}

// lo / hi of the group's windows, copied to LDS when they fit (then window w sits at index w - w0)
template <bool kLds>
__device__ __forceinline__ void stage_bounds(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int w0, int w1, int32_t* s_lo,
                                             int32_t* s_hi) {
    if (kLds) {
        for (int w = w0 + (int)threadIdx.x; w < w1; w += kBlock) { s_lo[w - w0] = lo[w]; s_hi[w - w0] = hi[w]; }
        __syncthreads();
    }
}

template <typename KeyT, bool kLds>
__global__ __launch_bounds__(kBlock) void k_roll_count(const KeyT* __restrict__ keys, const uint32_t* __restrict__ perm, int64_t m,
                                                      const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int w0, int w1,
                                                      int64_t max_run, const int32_t* __restrict__ flags, int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ report /* [w1 - w0 + 2]: difference array, status */) {
    __shared__ int32_t s_lo[kLds ? kRollLdsWindows : 1], s_hi[kLds ? kRollLdsWindows : 1], s_diff[kLds ? kRollLdsWindows + 1 : 1];
    const int wn = w1 - w0;
    if (kLds) {
        for (int w = threadIdx.x; w <= wn; w += kBlock) s_diff[w] = 0;
    }
    stage_bounds<kLds>(lo, hi, w0, w1, s_lo, s_hi);             // (its barrier also covers s_diff)
    const int32_t *L = kLds ? s_lo : lo, *H = kLds ? s_hi : hi;
    const int base = kLds ? w0 : 0;
    int32_t* diff = kLds ? s_diff : report;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int32_t bad = 0;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
        int a, b;
        head_range<KeyT>(keys, perm, j, L, H, base, w0, w1, a, b);
        const int c = b >= a ? b - a + 1 : 0;
        cnt[j] = c;
        if (c > 0) {
            atomicAdd(&diff[a - w0], 1);
            atomicAdd(&diff[b + 1 - w0], -1);
        }
        if (j >= max_run - 1 && keys[j] == keys[j - (max_run - 1)]) bad |= kRollLongRun;     // a run of max_run positions or more
    }
    if (kLds) {
        __syncthreads();
        for (int w = threadIdx.x; w <= wn; w += kBlock) {
            const int32_t d = s_diff[w];
            if (d != 0) atomicAdd(&report[w], d);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) bad |= flags[0];
    if (bad) atomicOr(&report[wn + 1], bad);
}

template <typename KeyT, bool kLds>
__global__ __launch_bounds__(kBlock) void k_roll_fill(const KeyT* __restrict__ keys, const uint32_t* __restrict__ perm, int64_t m,
                                                     const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int w0, int w1,
                                                     const int32_t* __restrict__ ptr, int64_t total, uint32_t* __restrict__ wkey,
                                                     uint32_t* __restrict__ pos) {
    __shared__ int32_t s_lo[kLds ? kRollLdsWindows : 1], s_hi[kLds ? kRollLdsWindows : 1];
    stage_bounds<kLds>(lo, hi, w0, w1, s_lo, s_hi);
    const int32_t *L = kLds ? s_lo : lo, *H = kLds ? s_hi : hi;
    const int base = kLds ? w0 : 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
        int a, b;
        head_range<KeyT>(keys, perm, j, L, H, base, w0, w1, a, b);
        const int64_t slot = ptr[j];
        for (int w = a; w <= b; ++w) {
            const int64_t s = slot + (w - a);
            if (s < total) {                  // (always, when `total` is the sum of this group's counts)
                wkey[s] = (uint32_t)(w - w0);
                pos[s] = (uint32_t)j;
            }
        }
    }
}

constexpr int kEmitBlock = 1024;           // k_roll_emit: 16 waves share the LDS stage of the windows' node maxima
constexpr int kEmitSpan = 64;              // windows (from the workgroup's first one on) that stage holds

template <typename KeyT>
__global__ __launch_bounds__(kEmitBlock) void k_roll_emit(const KeyT* __restrict__ keys, const uint32_t* __restrict__ perm, int64_t m, int bits,
                                                     const int32_t* __restrict__ hi, int w0, int wn, const uint32_t* __restrict__ wkey,
                                                     const uint32_t* __restrict__ pos, int64_t total, int64_t* __restrict__ out_src,
                                                     int64_t* __restrict__ out_dst, float* __restrict__ out_weight,
                                                     uint32_t* __restrict__ nn) {
    const int64_t q = (int64_t)blockIdx.x * kEmitBlock + threadIdx.x;
    int wl = -1;
    uint32_t top = 0;            // (unsigned: the largest admitted node, 2^32 - 2, gives 2^32 - 1; an int would wrap from node 2^31 - 1 on)
    if (q < total) {
        const int64_t j = pos[q];
        const int w = (int)wkey[q];
        if (j < m && w < wn) {
            wl = w;
            const KeyT key = keys[j];
            const int64_t u = (int64_t)((uint64_t)key >> bits), v = (int64_t)((uint64_t)key & ((1ull << bits) - 1ull));
            const int64_t end = hi[w0 + w];                      // events of the window are < end; perm[j] is one of them
            // first position p > j that leaves the run or the window.  perm ascends by at least 1 per position: p <= j + (end - perm[j])
            int64_t cap = j + (end - (int64_t)perm[j]);
            cap = cap > m ? m : cap;
            int64_t good = j, step = 1;
            while (good + step < cap && keys[good + step] == key && (int64_t)perm[good + step] < end) { good += step; step <<= 1; }
            int64_t first = good + 1, last = good + step < cap ? good + step : cap;
            while (first < last) {
                const int64_t mid = first + ((last - first) >> 1);
                if (keys[mid] == key && (int64_t)perm[mid] < end) first = mid + 1; else last = mid;
            }
            out_src[q] = u;
            out_dst[q] = v;
            out_weight[q] = (float)(first - j);
            top = (uint32_t)((u > v ? u : v) + 1);
        }
    }
    // num_nodes of the window.  Atomics of one address queue up (measured: about 7 ns each — a window of 10^5 edges kept the kernel waiting
    // for 1,500 of them), so the maxima are first merged per wave (its edges mostly belong to one window) and per workgroup in LDS (the
    // windows of kEmitBlock consecutive edges are the first one + 0 .. kEmitSpan - 1, or they go to memory directly): one atomic per
    // workgroup and window.
    __shared__ int s_first;
    __shared__ uint32_t s_top[kEmitSpan];
    if (threadIdx.x == 0) s_first = wl;
    if (threadIdx.x < kEmitSpan) s_top[threadIdx.x] = 0;
    __syncthreads();
    const int first_w = s_first;
    const int ref = __builtin_amdgcn_readfirstlane(wl);
    const bool uniform = __all(wl == ref || wl < 0);
    const uint32_t mine = uniform ? wave_max(wl < 0 ? 0u : top) : top;
    if (wl >= 0 && (!uniform || lane_id() == 0)) {            // (uniform with a live lane: lane 0 is live and speaks for the wave)
        const int d = wl - first_w;
        if (first_w >= 0 && d >= 0 && d < kEmitSpan) atomicMax(&s_top[d], mine); else atomicMax(&nn[wl], mine);
    }
    __syncthreads();
    if (threadIdx.x < kEmitSpan && s_top[threadIdx.x] > 0) atomicMax(&nn[first_w + threadIdx.x], s_top[threadIdx.x]);
}

static inline int roll_bits(int64_t num_nodes) { return bits_for((uint64_t)(num_nodes > 1 ? num_nodes - 1 : 1)); }

template <typename KeyT, typename TimeT>
static int rolling_group(const int64_t* edge_index, const TimeT* time, int64_t m, int64_t num_nodes, KeyT* keys_out, uint32_t* perm_out,
                         int32_t* flags, void* ws, size_t ws_bytes, hipStream_t st) {
    const int bits = roll_bits(num_nodes);
    Arena a(ws, ws_bytes);
    KeyT* raw = a.take<KeyT>(m);
    PP_REQUIRE(a.ok() && ws_bytes - a.used >= sort_ws_bytes(m, sizeof(KeyT)), PP_ERR_WORKSPACE, "pp_rolling_group: workspace too small");
    k_roll_keys<KeyT, TimeT><<<capped_grid(m, kBlock), kBlock, 0, st>>>(edge_index, edge_index + m, time, m, num_nodes, bits, raw, flags);
    PP_LAUNCH_CHECK();
    return sort_pairs<KeyT>(raw, nullptr, keys_out, perm_out, m, 0, 2 * bits, (char*)ws + a.used, ws_bytes - a.used, st);
}

struct RollFillWs {
    int32_t* ptr;
    uint32_t *wkey, *pos, *wkey_sorted, *pos_sorted;
    void *scan, *sort;
    size_t scan_bytes, sort_bytes, total_bytes;
};

static RollFillWs carve_roll_fill(void* ws, int64_t m, int64_t total) {
    Arena a(ws, (size_t)-1);
    RollFillWs w;
    w.ptr = a.take<int32_t>(m + 1);
    w.wkey = a.take<uint32_t>(total);
    w.pos = a.take<uint32_t>(total);
    w.wkey_sorted = a.take<uint32_t>(total);
    w.pos_sorted = a.take<uint32_t>(total);
    w.scan_bytes = scan_ws_bytes(m);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.sort_bytes = sort_ws_bytes(total, 4);
    w.sort = a.take<char>((int64_t)w.sort_bytes);
    w.total_bytes = a.used;
    return w;
}

template <typename KeyT>
static int rolling_count(const KeyT* keys, const uint32_t* perm, int64_t m, const int32_t* lo, const int32_t* hi, int w0, int w1,
                         int64_t max_run, const int32_t* flags, int32_t* cnt, int32_t* report, hipStream_t st) {
    PP_HIP(hipMemsetAsync(report, 0, (size_t)(w1 - w0 + 2) * sizeof(int32_t), st));
    if (w1 - w0 <= kRollLdsWindows)
        k_roll_count<KeyT, true><<<capped_grid(m, kBlock), kBlock, 0, st>>>(keys, perm, m, lo, hi, w0, w1, max_run, flags, cnt, report);
    else
        k_roll_count<KeyT, false><<<capped_grid(m, kBlock), kBlock, 0, st>>>(keys, perm, m, lo, hi, w0, w1, max_run, flags, cnt, report);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

template <typename KeyT>
static int rolling_fill(const KeyT* keys, const uint32_t* perm, int64_t m, int bits, const int32_t* lo, const int32_t* hi, int w0, int w1,
                        const int32_t* cnt, int64_t total, int64_t* out_src, int64_t* out_dst, float* out_weight, uint32_t* nn, void* ws,
                        hipStream_t st) {
    const int wn = w1 - w0;
    PP_HIP(hipMemsetAsync(nn, 0, (size_t)wn * sizeof(uint32_t), st));
    if (total == 0) return PP_OK;
    RollFillWs w = carve_roll_fill(ws, m, total);
    int rc = exclusive_scan<int32_t, int32_t>(cnt, m, w.ptr, true, nullptr, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    // (`total` is the sum of `cnt`, so every slot is written; should a caller pass a larger one, k_roll_emit skips what lies outside [0, m) x [0, wn))
    if (wn <= kRollLdsWindows)
        k_roll_fill<KeyT, true><<<capped_grid(m, kBlock), kBlock, 0, st>>>(keys, perm, m, lo, hi, w0, w1, w.ptr, total, w.wkey, w.pos);
    else
        k_roll_fill<KeyT, false><<<capped_grid(m, kBlock), kBlock, 0, st>>>(keys, perm, m, lo, hi, w0, w1, w.ptr, total, w.wkey, w.pos);
    PP_LAUNCH_CHECK();
    const uint32_t *wkey = w.wkey, *pos = w.pos;
    if (wn > 1) {      // one window: pair-major order is the window's order already
        rc = sort_pairs<uint32_t>(w.wkey, w.pos, w.wkey_sorted, w.pos_sorted, total, 0, bits_for((uint64_t)(wn - 1)), w.sort, w.sort_bytes, st);
        if (rc != PP_OK) return rc;
        wkey = w.wkey_sorted;
        pos = w.pos_sorted;
    }
    k_roll_emit<KeyT><<<(unsigned)ceil_div(total, kEmitBlock), kEmitBlock, 0, st>>>(keys, perm, m, bits, hi, w0, wn, wkey, pos, total, out_src, out_dst,
                                                                           out_weight, nn);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" {

int pp_rolling_key_bytes(int64_t num_nodes) { return 2 * roll_bits(num_nodes) <= 32 ? 4 : 8; }

size_t pp_rolling_group_ws_bytes(int64_t m, int64_t num_nodes) {
    const int kb = pp_rolling_key_bytes(num_nodes);
    return align_up((size_t)(m > 0 ? m : 1) * (size_t)kb) + sort_ws_bytes(m, kb);
}

int pp_rolling_group(const int64_t* edge_index, const void* time, int time_dtype, int64_t m, int64_t num_nodes, void* keys_out,
                     uint32_t* perm_out, int32_t* flags, void* ws, size_t ws_bytes, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(m >= 0 && m < (int64_t)0x7ffffff0, PP_ERR_TOO_LARGE, "pp_rolling_group: m=%lld outside [0, 2^31 - 16)", (long long)m);
    PP_REQUIRE(num_nodes >= 0 && num_nodes <= ((int64_t)1 << 32), PP_ERR_ARG, "pp_rolling_group: num_nodes=%lld outside [0, 2^32]", (long long)num_nodes);
    PP_REQUIRE(time_dtype == 1 || time_dtype == 3, PP_ERR_ARG, "pp_rolling_group: timestamps must be int64 (1) or float64 (3)");
    PP_REQUIRE(ws_bytes >= pp_rolling_group_ws_bytes(m, num_nodes), PP_ERR_WORKSPACE, "pp_rolling_group: workspace too small");
    PP_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (m == 0) return PP_OK;
    const bool wide = pp_rolling_key_bytes(num_nodes) == 8;
    if (time_dtype == 1) {
        return wide ? rolling_group<uint64_t, int64_t>(edge_index, (const int64_t*)time, m, num_nodes, (uint64_t*)keys_out, perm_out, flags, ws, ws_bytes, st)
                    : rolling_group<uint32_t, int64_t>(edge_index, (const int64_t*)time, m, num_nodes, (uint32_t*)keys_out, perm_out, flags, ws, ws_bytes, st);
    }
    return wide ? rolling_group<uint64_t, double>(edge_index, (const double*)time, m, num_nodes, (uint64_t*)keys_out, perm_out, flags, ws, ws_bytes, st)
                : rolling_group<uint32_t, double>(edge_index, (const double*)time, m, num_nodes, (uint32_t*)keys_out, perm_out, flags, ws, ws_bytes, st);
}

int pp_rolling_bounds(const void* time, int time_dtype, int64_t m, const void* starts, const void* ends, int64_t W, int32_t* lo, int32_t* hi,
                      pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(m >= 0 && m < (int64_t)0x7ffffff0, PP_ERR_TOO_LARGE, "pp_rolling_bounds: m=%lld outside [0, 2^31 - 16)", (long long)m);
    PP_REQUIRE(W >= 0 && W < (int64_t)0x7ffffff0, PP_ERR_TOO_LARGE, "pp_rolling_bounds: W=%lld outside [0, 2^31 - 16)", (long long)W);
    PP_REQUIRE(time_dtype == 1 || time_dtype == 3, PP_ERR_ARG, "pp_rolling_bounds: timestamps must be int64 (1) or float64 (3)");
    if (W == 0) return PP_OK;
    const unsigned g = (unsigned)ceil_div(W, kBlock);
    if (time_dtype == 1)
        k_roll_bounds<int64_t><<<g, kBlock, 0, st>>>((const int64_t*)time, m, (const int64_t*)starts, (const int64_t*)ends, W, lo, hi);
    else
        k_roll_bounds<double><<<g, kBlock, 0, st>>>((const double*)time, m, (const double*)starts, (const double*)ends, W, lo, hi);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

#define PP_ROLL_RANGE(what)                                                                                                              \
    PP_REQUIRE(m >= 0 && m < (int64_t)0x7ffffff0, PP_ERR_TOO_LARGE, what ": m=%lld outside [0, 2^31 - 16)", (long long)m);                \
    PP_REQUIRE(W >= 0 && W < (int64_t)0x7ffffff0, PP_ERR_TOO_LARGE, what ": W=%lld outside [0, 2^31 - 16)", (long long)W);                \
    PP_REQUIRE(0 <= w0 && w0 <= w1 && w1 <= W, PP_ERR_ARG, what ": windows [%lld, %lld) outside [0, %lld)", (long long)w0, (long long)w1, \
               (long long)W)

int pp_rolling_count(const void* keys, int key_bytes, const uint32_t* perm, int64_t m, const int32_t* lo, const int32_t* hi, int64_t W,
                     int64_t w0, int64_t w1, int64_t max_run, const int32_t* flags, int32_t* cnt, int32_t* report, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_ROLL_RANGE("pp_rolling_count");
    PP_REQUIRE(key_bytes == 4 || key_bytes == 8, PP_ERR_ARG, "pp_rolling_count: keys of 4 or 8 bytes");
    PP_REQUIRE(max_run >= 1, PP_ERR_ARG, "pp_rolling_count: max_run must be positive");
    if (m == 0) {
        PP_HIP(hipMemsetAsync(report, 0, (size_t)(w1 - w0 + 1) * sizeof(int32_t), st));
        PP_HIP(hipMemcpyAsync(report + (w1 - w0 + 1), flags, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        return PP_OK;
    }
    return key_bytes == 8 ? rolling_count<uint64_t>((const uint64_t*)keys, perm, m, lo, hi, (int)w0, (int)w1, max_run, flags, cnt, report, st)
                          : rolling_count<uint32_t>((const uint32_t*)keys, perm, m, lo, hi, (int)w0, (int)w1, max_run, flags, cnt, report, st);
}

size_t pp_rolling_fill_ws_bytes(int64_t m, int64_t total) { return carve_roll_fill(nullptr, m, total).total_bytes; }

int pp_rolling_fill(const void* keys, int key_bytes, const uint32_t* perm, int64_t m, int64_t num_nodes, const int32_t* lo, const int32_t* hi,
                    int64_t W, int64_t w0, int64_t w1, const int32_t* cnt, int64_t total, int64_t* out_src, int64_t* out_dst, float* out_weight,
                    uint32_t* num_nodes_out, void* ws, size_t ws_bytes, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_ROLL_RANGE("pp_rolling_fill");
    PP_REQUIRE(num_nodes >= 0 && num_nodes < ((int64_t)1 << 32), PP_ERR_ARG, "pp_rolling_fill: num_nodes=%lld outside [0, 2^32): a window's node count is 32 bits",
               (long long)num_nodes);
    PP_REQUIRE(key_bytes == pp_rolling_key_bytes(num_nodes), PP_ERR_ARG, "pp_rolling_fill: key width does not fit num_nodes");
    PP_REQUIRE(total >= 0 && total < (int64_t)0x7ffffff0, PP_ERR_TOO_LARGE, "pp_rolling_fill: total=%lld outside [0, 2^31 - 16)", (long long)total);
    PP_REQUIRE(m > 0 || total == 0, PP_ERR_ARG, "pp_rolling_fill: edges without events");
    PP_REQUIRE(ws_bytes >= pp_rolling_fill_ws_bytes(m, total), PP_ERR_WORKSPACE, "pp_rolling_fill: workspace too small");
    if (w1 == w0) return PP_OK;
    const int bits = roll_bits(num_nodes);
    return key_bytes == 8 ? rolling_fill<uint64_t>((const uint64_t*)keys, perm, m, bits, lo, hi, (int)w0, (int)w1, cnt, total, out_src, out_dst,
                                                   out_weight, num_nodes_out, ws, st)
                          : rolling_fill<uint32_t>((const uint32_t*)keys, perm, m, bits, lo, hi, (int)w0, (int)w1, cnt, total, out_src, out_dst,
                                                   out_weight, num_nodes_out, ws, st);
}

}  // extern "C"
