// pathpyg_amd — power-iteration centralities of a static Graph: eigenvector_centrality and katz_centrality.
//
// Reference: src/pathpyG/algorithms/centrality.py:327-356 forwards both names to networkx on a DiGraph copy of the graph; networkx 3.4 runs
// each iteration as nested Python dict loops.  Here an iteration is a PULL product over the predecessor lists of the distinct edges
// (Graph.simple_predecessors()), float64 values, int64 indices:
//   eigenvector: y[v] = x[v] + sum_u w(u, v) x[u];  norm = sqrt(sum y^2) or 1;  x' = y / norm;  err = sum |x' - x|
//   Katz       : x'[v] = alpha * (sum_u w(u, v) x[u]) + b[v];                   err = sum |x' - x|;  result x' * (1 / sqrt(sum x'^2))
// Launches of one iteration — 2 (Katz, no heavy row) to 4 (eigenvector with heavy rows), all plain, on one stream; no cooperative launch,
// no grid barrier, no floating-point atomic:
//   1. k_power_gather_groups: a row belongs to a GROUP of `width` lanes (work split of pp_rows.h); lane j adds entries j, j + width, ...
//      in order, the lanes fold by a butterfly.  A row of heavy_min entries or more is left to
//   2. k_power_gather_blocks (only if there are heavy rows): a whole workgroup per row, thread j adds entries j, j + 256, ...
//      Both write the new vector and one partial per workgroup: sum y^2, and for Katz sum |x' - x|.
//   3. k_power_scale (eigenvector only): folds the sum y^2 partials (every workgroup folds the same words in the same shape, so all hold the
//      same norm), writes x' = y / norm and one partial of sum |x' - x| per workgroup.  The error needs the global norm first; a pass of its
//      own over 24 bytes per node was chosen over folding the scale into the next gather, which would leave the iterate unnormalised when
//      the criterion holds and move the rounding of the division.
//   4. k_power_decide (one workgroup): folds the error partials, counts the iteration, swaps the buffers and sets `done` if err < threshold
//      (written that way: a NaN err is not below it).  Katz: also leaves 1 / sqrt(sum x'^2) for the final scaling.
// Every kernel reads state[kDone] first and returns once it is set: the iterate that first met the criterion stays where it is.  The host
// enqueues a batch of iterations, synchronises once and reads {done, iterations, buffer}.
// Determinism: the order of the adds inside a row depends on the row's length, `width` and heavy_min only.  Partials are folded in a fixed
// shape by workgroup index (thread t of the folding workgroup adds partials t, t + 256, ... in order, then wave butterfly, then the waves
// in order).  The grids depend on n, width and the number of heavy rows; the list of heavy rows is built by a scan, ascending.
#include "pp_common.h"
#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {

constexpr int64_t kPowerBatch = 16, kPowerBatchMin = 8;
constexpr int64_t kPowerLightParts = kMaxGrid - kBlock;   // workgroups of the light gather (and of k_power_scale)
constexpr int64_t kPowerHeavyParts = kBlock;              // workgroups of the heavy gather
constexpr int kStateWords = 8;                            // the shared words of pp_rows.h; none of its own

struct PowerArgs {
    const int64_t* col_ptr;        // [n + 1] predecessor lists
    const int64_t* row;            // [k]
    const double* weight;          // [k] or nullptr: every entry 1
    const double* beta;            // [n] or nullptr: beta_scalar
    int64_t n, k, heavy_min;
    int mode, normalized;
    double alpha, beta_scalar, threshold;
    double *x0, *x1;               // the iterate: state[kCur] says which is current (two fields, not an array: an index known only
                                   // at run time would put the by-value argument into scratch memory)
    double* y;                     // eigenvector: x + A^T x before the division
    double *sq_part, *err_part;    // [kMaxGrid] partials: light workgroups first, heavy ones from `light_parts` on
    int64_t light_parts, heavy_parts, scale_parts;
    const int32_t* heavy_list;     // ascending
    int64_t* state;                // kStateWords
    double* scale;                 // [1] Katz: the factor of the result
};

__device__ __forceinline__ double* power_buffer(const PowerArgs& a, int which) { return which ? a.x1 : a.x0; }

// entries lo + sub, lo + sub + step, ... of one predecessor list, added in that order
__device__ __forceinline__ double power_row_sum(const PowerArgs& a, const double* __restrict__ x, int64_t lo, int64_t hi, int sub, int step) {
    double s = 0.0;
    for (int64_t i = lo + sub; i < hi; i += step) {
        const int64_t u = load_stream(a.row + i);
        if ((uint64_t)u >= (uint64_t)a.n) continue;
        const double xu = x[u];
        s += a.weight ? load_stream(a.weight + i) * xu : xu;
    }
    return s;
}

// the new value of node v from its row sum
__device__ __forceinline__ double power_value(const PowerArgs& a, double xv, int64_t v, double sum) {
    if (a.mode == PP_POWER_EIGENVECTOR) return xv + sum;
    return a.alpha * sum + (a.beta ? a.beta[v] : a.beta_scalar);
}

__global__ __launch_bounds__(kBlock) void k_power_gather_groups(PowerArgs a, int width) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;                                                         // (uniform in the grid)
    const int cur = (int)(a.state[kCur] & 1);
    const double* x = power_buffer(a, cur);
    double* out = a.mode == PP_POWER_EIGENVECTOR ? a.y : power_buffer(a, cur ^ 1);
    const int sub = threadIdx.x & (width - 1);
    const int64_t per_block = kBlock / width, mine = threadIdx.x / width;
    double sq = 0.0, err = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < a.n; base += (int64_t)gridDim.x * per_block) {       // (uniform in the workgroup)
        const int64_t v = base + mine;
        const bool live = v < a.n;
        int64_t lo = 0, hi = 0;
        bool heavy = false;
        double s = 0.0;
        if (live) {
            row_span(a.col_ptr, v, a.k, lo, hi);
            heavy = hi - lo >= a.heavy_min;
            if (!heavy) s = power_row_sum(a, x, lo, hi, sub, width);
        }
        group_sum(width, s);                                                            // (partners share the node: both are here)
        if (live && sub == 0 && !heavy) {
            const double xv = x[v], y = power_value(a, xv, v, s);
            out[v] = y;
            sq += y * y;
            if (a.mode == PP_POWER_KATZ) err += fabs(y - xv);
        }
    }
    sq = block_sum_fixed(sq, scratch);
    err = block_sum_fixed(err, scratch);
    if (threadIdx.x == 0) { a.sq_part[blockIdx.x] = sq; a.err_part[blockIdx.x] = err; }
}

__global__ __launch_bounds__(kBlock) void k_power_gather_blocks(PowerArgs a) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;
    const int cur = (int)(a.state[kCur] & 1);
    const double* x = power_buffer(a, cur);
    double* out = a.mode == PP_POWER_EIGENVECTOR ? a.y : power_buffer(a, cur ^ 1);
    const int64_t heavy_count = a.state[kHeavyCount];
    double sq = 0.0, err = 0.0;                                                         // (thread 0's are the workgroup's)
    for (int64_t i = blockIdx.x; i < heavy_count; i += gridDim.x) {
        const int64_t v = a.heavy_list[i];
        if ((uint64_t)v >= (uint64_t)a.n) continue;                                     // (uniform in the workgroup)
        int64_t lo, hi;
        row_span(a.col_ptr, v, a.k, lo, hi);
        const double s = block_sum_fixed(power_row_sum(a, x, lo, hi, (int)threadIdx.x, kBlock), scratch);
        if (threadIdx.x == 0) {
            const double xv = x[v], y = power_value(a, xv, v, s);
            out[v] = y;
            sq += y * y;
            if (a.mode == PP_POWER_KATZ) err += fabs(y - xv);
        }
    }
    if (threadIdx.x == 0) { a.sq_part[a.light_parts + blockIdx.x] = sq; a.err_part[a.light_parts + blockIdx.x] = err; }
}

// eigenvector: x' = y / norm, one partial of sum |x' - x| per workgroup
__global__ __launch_bounds__(kBlock) void k_power_scale(PowerArgs a) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;
    const int cur = (int)(a.state[kCur] & 1);
    const double* x = power_buffer(a, cur);
    double* out = power_buffer(a, cur ^ 1);
    double norm = sqrt(fold_parts(a.sq_part, a.light_parts + a.heavy_parts, scratch));
    if (norm == 0.0) norm = 1.0;                                                        // (networkx: `hypot(...) or 1`; a NaN stays)
    double err = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) {
        const double xn = a.y[v] / norm;
        out[v] = xn;
        err += fabs(xn - x[v]);
    }
    err = block_sum_fixed(err, scratch);
    if (threadIdx.x == 0) a.err_part[blockIdx.x] = err;
}

__global__ __launch_bounds__(kBlock) void k_power_decide(PowerArgs a) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;
    const int64_t parts = a.mode == PP_POWER_EIGENVECTOR ? a.scale_parts : a.light_parts + a.heavy_parts;
    const double err = fold_parts(a.err_part, parts, scratch);
    double factor = 1.0;
    if (a.mode == PP_POWER_KATZ && a.normalized) {
        const double norm = sqrt(fold_parts(a.sq_part, parts, scratch));
        if (norm != 0.0) factor = 1.0 / norm;                                           // (networkx: a ZeroDivisionError leaves the factor 1)
    }
    if (threadIdx.x == 0) {
        a.state[kIters] += 1;
        a.state[kCur] ^= 1;
        if (err < a.threshold) {                                                        // (false for a NaN)
            a.state[kDone] = 1;
            a.scale[0] = factor;
        }
    }
}

// ------------------------------------------------------------------ set-up and result
__global__ __launch_bounds__(kBlock) void k_power_start(const double* __restrict__ start, double fill, int64_t n, double* __restrict__ x,
                                                       double* __restrict__ part) {
    __shared__ double scratch[kWavesPerBlock];
    double s = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const double t = start ? start[v] : fill;
        x[v] = t;
        s += t;
    }
    s = block_sum_fixed(s, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// eigenvector: x = start / sum(start)
__global__ __launch_bounds__(kBlock) void k_power_start_scale(double* __restrict__ x, int64_t n, const double* part, int64_t parts) {
    __shared__ double scratch[kWavesPerBlock];
    const double total = fold_parts(part, parts, scratch);
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) x[v] = x[v] / total;
}

__global__ __launch_bounds__(kBlock) void k_power_result(const PowerArgs a, double* __restrict__ values) {
    const double* x = power_buffer(a, (int)(a.state[kCur] & 1));
    const double f = a.scale[0];
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) values[v] = x[v] * f;
}

struct PowerWs {
    int64_t* state;
    double *scale, *sq_part, *err_part, *x0, *x1, *y;
    int32_t *flag, *pos, *heavy_list;
    void* scan;
    size_t scan_bytes, total;
};

static PowerWs carve_power(void* ws, int64_t n) {
    Arena a(ws, 0);
    PowerWs w{};
    w.state = a.take<int64_t>(kStateWords);
    w.scale = a.take<double>(1);
    w.sq_part = a.take<double>(kMaxGrid);
    w.err_part = a.take<double>(kMaxGrid);
    w.x0 = a.take<double>(n);
    w.x1 = a.take<double>(n);
    w.y = a.take<double>(n);
    w.flag = a.take<int32_t>(n);
    w.pos = a.take<int32_t>(n + 1);
    w.heavy_list = a.take<int32_t>(n);
    w.scan_bytes = scan_ws_bytes(n);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.total = a.used;
    return w;
}

}  // namespace pp

extern "C" {

int64_t pp_graph_power_heavy_min(void) { return pp::kHeavyMinDefault; }

size_t pp_graph_power_ws_bytes(int64_t n) { return pp::carve_power(nullptr, n > 0 ? n : 0).total; }

int pp_graph_power_iterate(const int64_t* col_ptr, const int64_t* row, const double* weight, int64_t n, int64_t k, int mode, double alpha,
                           const double* beta, double beta_scalar, const double* start, int normalized, double threshold, int64_t max_iter,
                           int64_t batch, int group, int64_t heavy_min, double* values, int64_t* iterations, int64_t* converged, int64_t* grids,
                           void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && k >= 0, PP_ERR_ARG, "pp_graph_power_iterate: negative size");
    PP_REQUIRE(n < (int64_t)0x7fffffff && k < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_power_iterate: size >= 2^31 - 1");
    PP_REQUIRE(mode == PP_POWER_EIGENVECTOR || mode == PP_POWER_KATZ, PP_ERR_ARG, "pp_graph_power_iterate: unknown mode %d", mode);
    PP_REQUIRE(iterations && converged && grids, PP_ERR_ARG, "pp_graph_power_iterate: iterations, converged and grids are required");
    PP_REQUIRE(max_iter >= 1, PP_ERR_ARG, "pp_graph_power_iterate: max_iter must be >= 1");
    PP_REQUIRE(batch == 0 || batch >= kPowerBatchMin, PP_ERR_ARG, "pp_graph_power_iterate: batch must be 0 or >= %lld", (long long)kPowerBatchMin);
    PP_REQUIRE(row_width_ok(group) && heavy_min >= 0, PP_ERR_ARG, "pp_graph_power_iterate: group must be 0 or a power of two up to 64");
    PP_REQUIRE(n == 0 || (values && col_ptr), PP_ERR_ARG, "pp_graph_power_iterate: values and col_ptr are required");
    PP_REQUIRE(k == 0 || row, PP_ERR_ARG, "pp_graph_power_iterate: row is required");
    PP_REQUIRE(ws_bytes >= pp_graph_power_ws_bytes(n), PP_ERR_WORKSPACE, "pp_graph_power_iterate: workspace too small");
    *iterations = 0;
    *converged = 0;
    grids[0] = grids[1] = 0;
    if (n == 0) return PP_OK;
    hipStream_t st = (hipStream_t)stream;
    const PowerWs w = carve_power(ws, n);
    const int width = row_width(group, n, k);
    const unsigned gn = capped_grid(n, kBlock, kPowerLightParts);
    int64_t host[kStateWords] = {0};

    PowerArgs a{};
    a.col_ptr = col_ptr; a.row = row; a.weight = weight; a.beta = beta; a.n = n; a.k = k;
    a.heavy_min = heavy_min > 0 ? heavy_min : kHeavyMinDefault;
    a.mode = mode; a.normalized = normalized; a.alpha = alpha; a.beta_scalar = beta_scalar; a.threshold = threshold;
    a.x0 = w.x0; a.x1 = w.x1; a.y = w.y; a.sq_part = w.sq_part; a.err_part = w.err_part;
    a.heavy_list = w.heavy_list; a.state = w.state; a.scale = w.scale;
    a.scale_parts = gn;

    // set-up: the heavy rows (ascending, by a scan), the start vector; one read-back
    PP_HIP(hipMemsetAsync(w.state, 0, kStateWords * sizeof(int64_t), st));
    int rc = heavy_rows_ascending(col_ptr, n, k, a.heavy_min, w.flag, w.pos, w.heavy_list, w.state + kHeavyCount, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    k_power_start<<<gn, kBlock, 0, st>>>(start, mode == PP_POWER_EIGENVECTOR ? 1.0 : 0.0, n, w.x0, w.err_part);
    PP_LAUNCH_CHECK();
    if (mode == PP_POWER_EIGENVECTOR) {
        k_power_start_scale<<<gn, kBlock, 0, st>>>(w.x0, n, w.err_part, (int64_t)gn);
        PP_LAUNCH_CHECK();
    }
    const double one = 1.0;
    PP_HIP(hipMemcpyAsync(w.scale, &one, sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(host, w.state, kStateWords * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    const int64_t heavy_count = host[kHeavyCount] < 0 ? 0 : (host[kHeavyCount] > n ? n : host[kHeavyCount]);

    const unsigned g_light = capped_grid(n, kBlock / width, kPowerLightParts);
    const unsigned g_heavy = heavy_count > 0 ? capped_grid(heavy_count, 1, kPowerHeavyParts) : 0;
    a.light_parts = g_light;
    a.heavy_parts = g_heavy;
    grids[0] = g_light;
    grids[1] = g_heavy;

    rc = run_batched(max_iter, batch > 0 ? batch : kPowerBatch, w.state, host, kStateWords, st, [&]() -> int {
        k_power_gather_groups<<<g_light, kBlock, 0, st>>>(a, width);
        PP_LAUNCH_CHECK();
        if (g_heavy > 0) {
            k_power_gather_blocks<<<g_heavy, kBlock, 0, st>>>(a);
            PP_LAUNCH_CHECK();
        }
        if (mode == PP_POWER_EIGENVECTOR) {
            k_power_scale<<<gn, kBlock, 0, st>>>(a);
            PP_LAUNCH_CHECK();
        }
        k_power_decide<<<1, kBlock, 0, st>>>(a);
        PP_LAUNCH_CHECK();
        return PP_OK;
    });
    if (rc != PP_OK) return rc;
    *iterations = host[kIters];
    *converged = host[kDone] ? 1 : 0;
    k_power_result<<<gn, kBlock, 0, st>>>(a, values);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
