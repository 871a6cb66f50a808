// pathpyg_amd — distributions on a Graph or on a layer of a MultiOrderModel: PageRank and the evolution of random-walk distributions, B
// of them at once (no reference counterpart: networkx.pagerank is not behind the reference's centrality forwarding; the iteration is
// networkx 3.4's, `x = alpha * (x @ A + sum(x[dangling]) * dangling_weights) + (1 - alpha) * p`).
//
// Layout: X is [n, B] float64 row-major, B a power of two up to 64: the B columns of a node are B contiguous doubles, so the lanes that
// work a row's columns read ONE contiguous line per predecessor (128 bytes at B = 16) where pp_graph_power.hip gathers 8 bytes.  A
// workgroup owns a RANGE of 256 nodes and works it in B passes of 256 / B rows; lane (r, c) of a pass sums row r for column c.
//
// One iteration is 2 plain launches, 3 with heavy rows, on one stream (no cooperative launch, no grid barrier, no floating-point atomic):
//   1. k_diff_heavy (only if there are heavy rows): a workgroup per row of heavy_min entries or more; leaves the row's sums in the output
//      block, where
//   2. k_diff_rows finds them: it sums the light rows, applies the mode's update to every (node, column), writes x' and three partials per
//      (range, column): sum |x' - x|, sum of x' over the dangling nodes (the next iteration's D), sum |x' - target|.
//   3. k_diff_decide, one workgroup per column: folds the column's partials over the ranges, counts the column's iteration, leaves D and
//      tvd, sets the column's `done` word if err < threshold (written that way: a NaN is not below it).  The last workgroup to arrive (an
//      integer counter) sets the run's `done` word once every column's is set.
// A column whose `done` word is set is copied, not updated: it keeps exactly the iterate that met the criterion, whatever the others do.
//
// The shapes of the sums — functions of a row's length, of n and of heavy_min only, never of B, of the other columns or of the grid:
//   row, fewer than heavy_min entries: entry i of the row goes into accumulator i mod 4, in order; the sum is (a0 + a1) + (a2 + a3);
//   row, heavy_min entries or more: chunks of 256 entries, each summed like a light row, added in order to 0.0;
//   over the nodes (err, D, tvd): per range of 256 nodes, the groups of 4 consecutive nodes are summed ((t0 + t1) + t2) + t3 and added in
//     order to 0.0 (nodes past n count 0.0); the ranges are folded by index by fold_parts (pp_rows.h): thread t adds ranges t, t + 256,
//     ... in order, wave butterfly, the waves in order.
// Nothing is contracted: every operation is one rounded float64 operation.
#include "pp_common.h"
#include "pp_internal.h"
#include "pp_rows.h"

#pragma clang fp contract(off)

namespace pp {

constexpr int kDiffRange = kBlock;                      // nodes per range (one partial per range and column)
constexpr int kDiffSub = 4;                             // nodes per group inside a range
constexpr int kDiffSubs = kDiffRange / kDiffSub;        // 64: the groups of one pass times the columns, whatever B is
constexpr int kDiffChunk = 256;                         // entries per chunk of a heavy row
constexpr int kDiffMaxB = 64;
constexpr int64_t kDiffBatch = 16;
constexpr int64_t kDiffLimit = 0x7fffffff;
constexpr int64_t kDiffMaxBytes = (int64_t)1 << 47;     // no device addresses more

enum { kDiffDoneAt = kStateShared, kDiffItersAt = kDiffDoneAt + kDiffMaxB, kDiffArrived = kDiffItersAt + kDiffMaxB, kDiffWords = kDiffArrived + 1 };
enum { kDiffSum = 2, kDiffMeasure = 3 };                // kernel modes beside PP_DIFFUSION_PAGERANK / _WALK

struct DiffArgs {
    const int64_t* ptr;            // [n + 1] pull lists
    const int64_t* src;            // [k]
    const double* prob;            // [k] or nullptr: every entry 1
    const uint8_t* dangling;       // [n]
    const double *p, *d;           // [n, B] PageRank: personalisation and dangling weights
    const double* target;          // [n] or nullptr
    int64_t n, n_src, k, heavy_min, ranges;
    int B, log2B;
    double alpha, one_minus_alpha, lazy, one_minus_lazy, threshold;
    double* part;                  // [3, B, ranges]
    double* D;                     // [B]
    double* tvd;                   // [rows, B] or nullptr
    const int32_t* heavy_list;     // ascending
    int64_t heavy_count;
    int64_t* state;                // kDiffWords
};

// entries [lo, hi) in order, entry i into accumulator (i - lo) mod 4; (a0 + a1) + (a2 + a3)
__device__ __forceinline__ double diff_term(const DiffArgs& a, const double* __restrict__ x, int c, int64_t i) {
    const int64_t u = a.src[i];
    if ((uint64_t)u >= (uint64_t)a.n_src) return 0.0;
    const double xu = x[u * a.B + c];
    return a.prob ? a.prob[i] * xu : xu;
}
__device__ __forceinline__ double diff_span_sum(const DiffArgs& a, const double* __restrict__ x, int c, int64_t lo, int64_t hi) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t i = lo;
    for (; i + 4 <= hi; i += 4) {
        const double t0 = diff_term(a, x, c, i), t1 = diff_term(a, x, c, i + 1), t2 = diff_term(a, x, c, i + 2), t3 = diff_term(a, x, c, i + 3);
        a0 += t0; a1 += t1; a2 += t2; a3 += t3;
    }
    if (i < hi) a0 += diff_term(a, x, c, i);
    if (i + 1 < hi) a1 += diff_term(a, x, c, i + 1);
    if (i + 2 < hi) a2 += diff_term(a, x, c, i + 2);
    return (a0 + a1) + (a2 + a3);
}

// the rows of heavy_min entries or more: out[v, c] = the row's sum
__global__ __launch_bounds__(kBlock) void k_diff_heavy(DiffArgs a, const double* __restrict__ in, double* __restrict__ out, int check_done) {
    __shared__ double lds[kBlock];
    if (check_done && a.state[kDone]) return;                                           // (uniform in the grid)
    const int c = threadIdx.x & (a.B - 1), j = threadIdx.x >> a.log2B, workers = kBlock >> a.log2B;
    for (int64_t i = blockIdx.x; i < a.heavy_count; i += gridDim.x) {
        const int64_t v = a.heavy_list[i];
        if ((uint64_t)v >= (uint64_t)a.n) continue;                                     // (uniform in the workgroup)
        int64_t lo, hi;
        row_span(a.ptr, v, a.k, lo, hi);
        const int64_t chunks = (hi - lo + kDiffChunk - 1) / kDiffChunk;
        double total = 0.0;                                                             // (threads below B: their column's)
        for (int64_t base = 0; base < chunks; base += workers) {
            const int64_t ch = base + j;
            double s = 0.0;
            if (ch < chunks) {
                const int64_t clo = lo + ch * kDiffChunk, chi = clo + kDiffChunk < hi ? clo + kDiffChunk : hi;
                s = diff_span_sum(a, in, c, clo, chi);
            }
            lds[threadIdx.x] = s;                                                       // (= [j][c])
            __syncthreads();
            if ((int)threadIdx.x < a.B) {
                const int64_t left = chunks - base;
                const int count = left < workers ? (int)left : workers;
                for (int jj = 0; jj < count; ++jj) total += lds[(jj << a.log2B) + threadIdx.x];
            }
            __syncthreads();
        }
        if ((int)threadIdx.x < a.B) out[v * a.B + threadIdx.x] = total;
    }
}

// MODE PP_DIFFUSION_PAGERANK / _WALK: one iteration in -> out with its partials.  kDiffSum: out[v, c] = the row sum (projection).
// kDiffMeasure: the D and tvd partials of `in` itself (the start).
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_diff_rows(DiffArgs a, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double lds[3][kBlock];
    __shared__ double sub[3][kDiffSubs];
    constexpr bool kIterates = MODE == PP_DIFFUSION_PAGERANK || MODE == PP_DIFFUSION_WALK;
    constexpr bool kFolds = MODE != kDiffSum;
    if (kIterates && a.state[kDone]) return;                                            // (uniform in the grid)
    const int B = a.B, c = threadIdx.x & (B - 1), r = threadIdx.x >> a.log2B, rows = kBlock >> a.log2B;
    const bool frozen = kIterates && a.state[kDiffDoneAt + c] != 0;
    const double Dc = MODE == PP_DIFFUSION_PAGERANK ? a.D[c] : 0.0;
    for (int64_t range = blockIdx.x; range < a.ranges; range += gridDim.x) {            // (uniform in the workgroup)
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;                                      // (threads below B: their column's)
        for (int pass = 0; pass < B; ++pass) {
            const int64_t v = range * kDiffRange + (int64_t)pass * rows + r;
            double e = 0.0, dd = 0.0, tt = 0.0;
            if (v < a.n) {
                const int64_t at = v * B + c;
                double s = 0.0;
                if (MODE != kDiffMeasure) {
                    int64_t lo, hi;
                    row_span(a.ptr, v, a.k, lo, hi);
                    const bool heavy = hi - lo >= a.heavy_min;
                    if (MODE == kDiffSum) {
                        if (!heavy) out[at] = diff_span_sum(a, in, c, lo, hi);
                    } else {
                        s = heavy ? out[at] : diff_span_sum(a, in, c, lo, hi);          // (k_diff_heavy left it there)
                    }
                }
                if (kFolds) {
                    const double xv = in[at];
                    const bool dang = a.dangling[v] != 0;
                    double xn = xv;
                    if (MODE == PP_DIFFUSION_PAGERANK) {
                        const double inner = s + Dc * a.d[at];
                        xn = a.alpha * inner + a.one_minus_alpha * a.p[at];
                    } else if (MODE == PP_DIFFUSION_WALK) {
                        const double moved = s + (dang ? xv : 0.0);
                        xn = a.lazy * xv + a.one_minus_lazy * moved;
                    }
                    if (frozen) xn = xv;
                    if (kIterates) out[at] = xn;
                    e = fabs(xn - xv);
                    dd = dang ? xn : 0.0;
                    if (a.target) tt = fabs(xn - a.target[v]);
                }
            }
            if (kFolds) {
                lds[0][threadIdx.x] = e;                                                // (= [row of the pass][c])
                lds[1][threadIdx.x] = dd;
                lds[2][threadIdx.x] = tt;
                __syncthreads();
                if (threadIdx.x < kDiffSubs) {                                          // group g of the pass, column cc: 64 of them, whatever B is
                    const int g = threadIdx.x >> a.log2B, cc = threadIdx.x & (B - 1), first = ((g * kDiffSub) << a.log2B) + cc;
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        sub[q][threadIdx.x] = ((lds[q][first] + lds[q][first + B]) + lds[q][first + 2 * B]) + lds[q][first + 3 * B];
                }
                __syncthreads();
                if ((int)threadIdx.x < B) {
                    const int groups = rows / kDiffSub;
                    for (int g = 0; g < groups; ++g) {
                        acc0 += sub[0][(g << a.log2B) + threadIdx.x];
                        acc1 += sub[1][(g << a.log2B) + threadIdx.x];
                        acc2 += sub[2][(g << a.log2B) + threadIdx.x];
                    }
                }
            }
        }
        if (kFolds && (int)threadIdx.x < B) {
            a.part[((int64_t)0 * B + threadIdx.x) * a.ranges + range] = acc0;
            a.part[((int64_t)1 * B + threadIdx.x) * a.ranges + range] = acc1;
            a.part[((int64_t)2 * B + threadIdx.x) * a.ranges + range] = acc2;
        }
    }
}

// one workgroup per column.  start: the D and tvd of the start block (row 0 of tvd), nothing is counted
__global__ __launch_bounds__(kBlock) void k_diff_decide(DiffArgs a, int64_t tvd_row, int start) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;                                                         // (uniform in the grid)
    const int c = blockIdx.x;
    const bool frozen = a.state[kDiffDoneAt + c] != 0;                                  // (uniform in the workgroup)
    double err = 0.0, D = 0.0, tv = 0.0;
    if (!frozen) {
        if (!start) err = fold_parts(a.part + ((int64_t)0 * a.B + c) * a.ranges, a.ranges, scratch);
        D = fold_parts(a.part + ((int64_t)1 * a.B + c) * a.ranges, a.ranges, scratch);
        if (a.target) tv = fold_parts(a.part + ((int64_t)2 * a.B + c) * a.ranges, a.ranges, scratch);
    }
    if (threadIdx.x != 0) return;
    if (!frozen) {
        a.D[c] = D;
        if (a.tvd && a.target) a.tvd[tvd_row * a.B + c] = 0.5 * tv;
        if (!start) {
            a.state[kDiffItersAt + c] += 1;
            if (err < a.threshold) a.state[kDiffDoneAt + c] = 1;                        // (false for a NaN)
        }
    }
    if (start) return;
    __threadfence();
    const unsigned long long arrived = atomicAdd((unsigned long long*)(a.state + kDiffArrived), 1ull);
    if (arrived + 1 == gridDim.x) {                                                     // the last column to arrive: every `done` word is written
        __threadfence();
        a.state[kDiffArrived] = 0;
        bool all = true;
        for (int cc = 0; cc < a.B; ++cc)
            all &= __hip_atomic_load(a.state + kDiffDoneAt + cc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        a.state[kIters] += 1;
        if (all) a.state[kDone] = 1;
    }
}

// ------------------------------------------------------------------ the transition table
// T_u = the left-to-right sum of u's merged entries (weight in successor order; nullptr: ones); dangling[u] = !(T_u > 0)
__global__ __launch_bounds__(kBlock) void k_diff_totals(const int64_t* __restrict__ row_ptr, const double* __restrict__ weight, int64_t n, int64_t k,
                                                       double* __restrict__ total, uint8_t* __restrict__ dangling, int32_t* __restrict__ bad) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int64_t lo, hi;
        row_span(row_ptr, v, k, lo, hi);
        double s = 0.0;
        bool wrong = false;
        for (int64_t j = lo; j < hi; ++j) {
            const double w = weight ? weight[j] : 1.0;
            wrong |= !(w >= 0.0) || w > 1.7976931348623157e308;                        // negative, NaN or infinite
            s += w;
        }
        total[v] = s;
        dangling[v] = !(s > 0.0);
        wrong |= s > 1.7976931348623157e308;
        if (wrong) bad[0] = 1;                                                        // (every lane that finds one stores the same 1)
    }
}

// prob[j] = w / T_u of pull entry j (u = src[j], w = the weight of successor entry perm[j]): one rounded division; 0 where T_u is 0
__global__ __launch_bounds__(kBlock) void k_diff_probs(const int64_t* __restrict__ src, const int64_t* __restrict__ perm, const double* __restrict__ weight,
                                                      const double* __restrict__ total, int64_t n, int64_t k, double* __restrict__ prob) {
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < k; j += (int64_t)gridDim.x * kBlock) {
        const int64_t u = src[j], q = perm[j];
        double pr = 0.0;
        if ((uint64_t)u < (uint64_t)n && (uint64_t)q < (uint64_t)k) {
            const double T = total[u], w = weight ? weight[q] : 1.0;
            if (T > 0.0) pr = w / T;
        }
        prob[j] = pr;
    }
}

static unsigned diff_grid(int64_t items, int64_t per_block) {
    int64_t g = ceil_div(items > 0 ? items : 1, per_block);
    const int64_t share = shared_grid(kMaxGrid);
    if (g > share) g = share;
    note_persistent_grid(g);
    return (unsigned)g;
}

static bool diff_width_ok(int64_t B) { return B >= 1 && B <= kDiffMaxB && (B & (B - 1)) == 0; }
static int diff_log2(int B) {
    int l = 0;
    while ((1 << l) < B) ++l;
    return l;
}

struct DiffWs {
    int64_t* state;
    double *D, *part;
    int32_t *flag, *pos, *heavy_list;
    void* scan;
    size_t scan_bytes, total;
};

static DiffWs carve_diff(void* ws, int64_t rows, int64_t B) {
    Arena a(ws, 0);
    DiffWs w{};
    w.state = a.take<int64_t>(kDiffWords);
    w.D = a.take<double>(kDiffMaxB);
    w.part = a.take<double>(3 * B * ceil_div(rows > 0 ? rows : 1, kDiffRange));
    w.flag = a.take<int32_t>(rows);
    w.pos = a.take<int32_t>(rows + 1);
    w.heavy_list = a.take<int32_t>(rows);
    w.scan_bytes = scan_ws_bytes(rows);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.total = a.used;
    return w;
}

// the heavy rows of `ptr`, ascending, and their number on the host (one synchronisation)
static int diff_heavy_rows(const int64_t* ptr, int64_t rows, int64_t k, int64_t heavy_min, const DiffWs& w, int64_t* count, hipStream_t st) {
    int64_t host[kDiffWords] = {0};
    PP_HIP(hipMemsetAsync(w.state, 0, kDiffWords * sizeof(int64_t), st));
    const int rc = heavy_rows_ascending(ptr, rows, k, heavy_min, w.flag, w.pos, w.heavy_list, w.state + kHeavyCount, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    PP_HIP(hipMemcpyAsync(host, w.state, kDiffWords * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    *count = host[kHeavyCount] < 0 ? 0 : (host[kHeavyCount] > rows ? rows : host[kHeavyCount]);
    return PP_OK;
}

}  // namespace pp

extern "C" {

int64_t pp_diffusion_heavy_min(void) { return pp::kHeavyMinDefault; }

int pp_diffusion_check_sizes(int64_t n, int64_t k, int64_t B, int64_t kept) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && k >= 0 && kept >= 1, PP_ERR_ARG, "pp_diffusion: negative size, or no block to keep");
    PP_REQUIRE(diff_width_ok(B), PP_ERR_ARG, "pp_diffusion: the padded width must be a power of two up to %d, got %lld", kDiffMaxB, (long long)B);
    PP_REQUIRE(n < kDiffLimit && k < kDiffLimit, PP_ERR_TOO_LARGE, "pp_diffusion: 2^31 - 1 nodes or entries, or more");
    const int64_t block = n * B * (int64_t)sizeof(double);                              // (< 2^40)
    PP_REQUIRE(block == 0 || kept <= kDiffMaxBytes / block, PP_ERR_TOO_LARGE, "pp_diffusion: %lld blocks of %lld bytes cannot be allocated",
               (long long)kept, (long long)block);
    return PP_OK;
}

int pp_diffusion_table(const int64_t* row_ptr, const double* weight, const int64_t* src, const int64_t* perm, int64_t n, int64_t k, double* total,
                       double* prob, uint8_t* dangling, int32_t* bad, pp_stream_t stream) {
    using namespace pp;
    const int rc = pp_diffusion_check_sizes(n, k, 1, 1);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(bad && (n == 0 || (row_ptr && total && dangling)) && (k == 0 || (src && perm && prob)), PP_ERR_ARG, "pp_diffusion_table: null pointer");
    hipStream_t st = (hipStream_t)stream;
    PP_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n == 0) return PP_OK;
    k_diff_totals<<<diff_grid(n, kBlock), kBlock, 0, st>>>(row_ptr, weight, n, k, total, dangling, bad);
    PP_LAUNCH_CHECK();
    if (k > 0) {
        k_diff_probs<<<diff_grid(k, kBlock), kBlock, 0, st>>>(src, perm, weight, total, n, k, prob);
        PP_LAUNCH_CHECK();
    }
    return PP_OK;
}

size_t pp_diffusion_ws_bytes(int64_t rows, int64_t B) {
    return pp::carve_diff(nullptr, rows > 0 ? rows : 0, pp::diff_width_ok(B) ? B : pp::kDiffMaxB).total;
}

int pp_diffusion_run(const int64_t* col_ptr, const int64_t* src, const double* prob, const uint8_t* dangling, int64_t n, int64_t k, int B, int live,
                     int mode, double alpha, double lazy, const double* p, const double* d, const double* target, double* X, int64_t kept,
                     double threshold, int64_t max_iter, int64_t batch, int64_t heavy_min, int64_t* iterations, int64_t* converged, int64_t* where,
                     double* tvd, int64_t* grids, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    const int rc0 = pp_diffusion_check_sizes(n, k, B, kept);
    if (rc0 != PP_OK) return rc0;
    PP_REQUIRE(mode == PP_DIFFUSION_PAGERANK || mode == PP_DIFFUSION_WALK, PP_ERR_ARG, "pp_diffusion_run: unknown mode %d", mode);
    PP_REQUIRE(live >= 1 && live <= B, PP_ERR_ARG, "pp_diffusion_run: the live columns are 1 .. B");
    PP_REQUIRE(max_iter >= 0 && max_iter < kDiffLimit && batch >= 0 && heavy_min >= 0, PP_ERR_ARG, "pp_diffusion_run: bad max_iter, batch or heavy_min");
    PP_REQUIRE(kept == 2 || kept == max_iter + 1, PP_ERR_ARG, "pp_diffusion_run: X holds 2 blocks, or max_iter + 1 to keep every iterate");
    PP_REQUIRE(iterations && converged && where && grids, PP_ERR_ARG, "pp_diffusion_run: iterations, converged, where and grids are required");
    PP_REQUIRE(n == 0 || (col_ptr && dangling && X), PP_ERR_ARG, "pp_diffusion_run: col_ptr, dangling and X are required");
    PP_REQUIRE(k == 0 || (src && prob), PP_ERR_ARG, "pp_diffusion_run: src and prob are required");
    PP_REQUIRE(mode != PP_DIFFUSION_PAGERANK || n == 0 || (p && d), PP_ERR_ARG, "pp_diffusion_run: PageRank needs p and d");
    PP_REQUIRE(!tvd || target, PP_ERR_ARG, "pp_diffusion_run: tvd needs a target");
    PP_REQUIRE(ws_bytes >= pp_diffusion_ws_bytes(n, B), PP_ERR_WORKSPACE, "pp_diffusion_run: workspace too small");
    for (int c = 0; c < B; ++c) iterations[c] = converged[c] = 0;
    *where = 0;
    grids[0] = grids[1] = 0;
    if (n == 0) return PP_OK;
    hipStream_t st = (hipStream_t)stream;
    const DiffWs w = carve_diff(ws, n, B);

    DiffArgs a{};
    a.ptr = col_ptr; a.src = src; a.prob = prob; a.dangling = dangling; a.p = p; a.d = d; a.target = target;
    a.n = n; a.n_src = n; a.k = k; a.heavy_min = heavy_min > 0 ? heavy_min : kHeavyMinDefault;
    a.ranges = ceil_div(n, kDiffRange);
    a.B = B; a.log2B = diff_log2(B);
    a.alpha = alpha; a.one_minus_alpha = 1.0 - alpha; a.lazy = lazy; a.one_minus_lazy = 1.0 - lazy; a.threshold = threshold;
    a.part = w.part; a.D = w.D; a.tvd = tvd; a.heavy_list = w.heavy_list; a.state = w.state;

    int rc = diff_heavy_rows(col_ptr, n, k, a.heavy_min, w, &a.heavy_count, st);
    if (rc != PP_OK) return rc;
    int64_t host[kDiffWords] = {0};
    for (int c = live; c < B; ++c) host[kDiffDoneAt + c] = 1;                           // the padding columns never count
    host[kHeavyCount] = a.heavy_count;
    PP_HIP(hipMemcpyAsync(w.state, host, kDiffWords * sizeof(int64_t), hipMemcpyHostToDevice, st));
    PP_HIP(hipStreamSynchronize(st));                                                   // (`host` is reused below)

    const unsigned g_rows = diff_grid(a.ranges, 1);
    const unsigned g_heavy = a.heavy_count > 0 ? capped_grid(a.heavy_count, 1, kBlock) : 0;
    grids[0] = g_rows;
    grids[1] = g_heavy;
    const int64_t block = n * B;

    // D and tvd of the start
    k_diff_rows<kDiffMeasure><<<g_rows, kBlock, 0, st>>>(a, X, nullptr);
    PP_LAUNCH_CHECK();
    k_diff_decide<<<B, kBlock, 0, st>>>(a, 0, 1);
    PP_LAUNCH_CHECK();

    int64_t enqueued = 0;
    rc = run_batched(max_iter, batch > 0 ? batch : kDiffBatch, w.state, host, kDiffWords, st, [&]() -> int {
        const double* in = X + (kept == 2 ? (enqueued & 1) : enqueued) * block;
        double* out = X + (kept == 2 ? ((enqueued + 1) & 1) : enqueued + 1) * block;
        if (g_heavy > 0) {
            k_diff_heavy<<<g_heavy, kBlock, 0, st>>>(a, in, out, 1);
            PP_LAUNCH_CHECK();
        }
        if (mode == PP_DIFFUSION_PAGERANK)
            k_diff_rows<PP_DIFFUSION_PAGERANK><<<g_rows, kBlock, 0, st>>>(a, in, out);
        else
            k_diff_rows<PP_DIFFUSION_WALK><<<g_rows, kBlock, 0, st>>>(a, in, out);
        PP_LAUNCH_CHECK();
        k_diff_decide<<<B, kBlock, 0, st>>>(a, enqueued + 1, 0);
        PP_LAUNCH_CHECK();
        ++enqueued;
        return PP_OK;
    });
    if (rc != PP_OK) return rc;
    if (max_iter == 0) PP_HIP(hipStreamSynchronize(st));
    const int64_t ran = max_iter == 0 ? 0 : host[kIters];
    for (int c = 0; c < live; ++c) {
        iterations[c] = host[kDiffItersAt + c];
        converged[c] = host[kDiffDoneAt + c] ? 1 : 0;
    }
    *where = kept == 2 ? (ran & 1) : ran;
    return PP_OK;
}

int pp_diffusion_project(const int64_t* ptr, const int64_t* idx, int64_t rows, int64_t n_src, int64_t k, const double* x, int B, double* out,
                         int64_t heavy_min, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    int rc = pp_diffusion_check_sizes(rows, k, B, 1);
    if (rc == PP_OK) rc = pp_diffusion_check_sizes(n_src, k, B, 1);
    if (rc != PP_OK) return rc;
    PP_REQUIRE(heavy_min >= 0, PP_ERR_ARG, "pp_diffusion_project: negative heavy_min");
    PP_REQUIRE(rows == 0 || (ptr && out), PP_ERR_ARG, "pp_diffusion_project: ptr and out are required");
    PP_REQUIRE(k == 0 || (idx && x), PP_ERR_ARG, "pp_diffusion_project: idx and x are required");
    PP_REQUIRE(ws_bytes >= pp_diffusion_ws_bytes(rows, B), PP_ERR_WORKSPACE, "pp_diffusion_project: workspace too small");
    if (rows == 0) return PP_OK;
    hipStream_t st = (hipStream_t)stream;
    const DiffWs w = carve_diff(ws, rows, B);
    DiffArgs a{};
    a.ptr = ptr; a.src = idx; a.n = rows; a.n_src = n_src; a.k = k; a.heavy_min = heavy_min > 0 ? heavy_min : kHeavyMinDefault;
    a.ranges = ceil_div(rows, kDiffRange);
    a.B = B; a.log2B = diff_log2(B);
    a.heavy_list = w.heavy_list; a.state = w.state;
    rc = diff_heavy_rows(ptr, rows, k, a.heavy_min, w, &a.heavy_count, st);
    if (rc != PP_OK) return rc;
    if (a.heavy_count > 0) {
        k_diff_heavy<<<capped_grid(a.heavy_count, 1, kBlock), kBlock, 0, st>>>(a, x, out, 0);
        PP_LAUNCH_CHECK();
    }
    k_diff_rows<kDiffSum><<<diff_grid(a.ranges, 1), kBlock, 0, st>>>(a, x, out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
