// pathpyg_amd — the ascending list of heavy rows (pp_rows.h) for the kernels whose float64 sums depend on the order in which the heavy
// rows are handed to workgroups: flags, an exclusive scan, a scatter.  One writer per word, no atomic; the same list on every run.
#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {

__global__ __launch_bounds__(kBlock) void k_heavy_flags(const int64_t* __restrict__ ptr, int64_t n, int64_t total, int64_t heavy_min,
                                                       int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int64_t lo, hi;
        row_span(ptr, v, total, lo, hi);
        flag[v] = hi - lo >= heavy_min;
    }
}

__global__ __launch_bounds__(kBlock) void k_heavy_list(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int64_t n,
                                                      int32_t* __restrict__ list) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const int32_t p = pos[v];
        if (flag[v] && (uint64_t)p < (uint64_t)n) list[p] = (int32_t)v;                 // (a scan: ascending, one writer per word)
    }
}

int heavy_rows_ascending(const int64_t* ptr, int64_t n, int64_t total, int64_t heavy_min, int32_t* flag, int32_t* pos, int32_t* list,
                         int64_t* count_dev, void* scan_ws, size_t scan_bytes, hipStream_t st) {
    const unsigned g = capped_grid(n, kBlock);
    k_heavy_flags<<<g, kBlock, 0, st>>>(ptr, n, total, heavy_min, flag);
    PP_LAUNCH_CHECK();
    const int rc = exclusive_scan<int32_t, int32_t>(flag, n, pos, true, count_dev, scan_ws, scan_bytes, st);
    if (rc != PP_OK) return rc;
    k_heavy_list<<<g, kBlock, 0, st>>>(flag, pos, n, list);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // namespace pp
