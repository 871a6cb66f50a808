// pathpyg_amd — sizes of the intersection of two sorted neighbour lists: closed triads, clustering coefficients, node similarities.
//
// Reference: src/pathpyG/statistics/clustering.py (closed_triads: a doubly nested Python loop over successor lists per node, called once per
// node by avg_clustering_coefficient), node_similarities.py (two Python sets per pair; cosine_similarity densifies the adjacency matrix) and
// degrees.py (degree_assortativity).  Here all of them are one primitive on the SIMPLE successor structure of the graph (row_ptr [n + 1],
// col strictly increasing inside a row, mult = the number of stored parallel edges behind an entry):
//   meet(v, w) = |S(v) ∩ S(w)|, with  dot = sum of mult_v(u) mult_w(u)  and  aa = sum of table[stored out-degree of u]  over the common u.
// Over the entries e = (v, x) of the structure it is the number of closed triads (x, y) of v that start with x — the reference's set, self-loops
// included: x = v and y = x are members of the lists like any other — and the per-node count is a difference of the scan of these numbers.
//
// Work split (pp_rows.h): a task (one pair of lists) belongs to a GROUP of `width` lanes (a power of two, 1 .. 64, one value per launch,
// chosen by the host from the mean length of a list).  Lane r of the group takes the entries r, r + width, ... of the SHORTER list and
// bisects the longer one; a lane's keys ascend, so every search starts where the last one ended.  Cost: min(d) / width searches of log(max d) steps per lane.  A task
// whose shorter list has `heavy_min` entries or more is not walked by its group: the group's first lane appends it to a list (one integer
// atomic), and a second launch gives every listed task a whole workgroup.  The list's order depends on scheduling; no output does: every task
// writes its own words, the integers are exact and the float64 sum `aa` has a fixed shape for given width and heavy_min — a lane adds its terms
// in ascending u, the lanes are folded by a butterfly, the waves of a workgroup in wave order.  No floating-point atomics anywhere.
// Node indices outside [0, n) are never dereferenced (such a task meets an empty list) and a row pointer is clamped to the entry array.
#include "pp_common.h"
#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {

struct MeetArgs {
    const int64_t *row_ptr, *col, *mult;   // the simple structure; mult == nullptr: every multiplicity is 1
    int64_t n, ms;
    const int64_t *first, *second;         // task t meets the rows first[t] and second[t]
    int64_t tasks;
    const int64_t* deg_ptr;                // [n + 1] row pointers of the STORED edges (out-degrees with parallel edges); read only with a table
    const double* table;                   // [table_len] term of a common neighbour by its stored out-degree; nullptr: no aa
    int64_t table_len;
    int64_t *common, *dot;                 // [tasks]; dot may be nullptr
    double* aa;                            // [tasks] or nullptr
    int64_t* sizes;                        // [2, tasks] or nullptr: the lengths of the two lists
    int64_t* heavy_list;                   // [tasks]
    unsigned long long* heavy_count;
};

struct Meet {
    int64_t common, dot;
    double aa;
};

__device__ __forceinline__ void row_bounds(const MeetArgs& a, int64_t v, int64_t& lo, int64_t& hi) {
    lo = hi = 0;
    if ((uint64_t)v < (uint64_t)a.n) row_span(a.row_ptr, v, a.ms, lo, hi);               // (a node outside [0, n): an empty list)
}

// The walk shared by every kernel below: lane `rank` of `width` takes every width-th entry of [a0, a1) and bisects [b0, b1).
__device__ __forceinline__ void meet_lists(const MeetArgs& a, int64_t a0, int64_t a1, int64_t b0, int64_t b1, int rank, int width, Meet& acc) {
    int64_t from = b0;
    for (int64_t i = a0 + rank; i < a1; i += width) {
        const int64_t u = a.col[i];
        const int64_t j = lower_bound_dev(a.col, from, b1, u);
        from = j;
        if (j >= b1 || a.col[j] != u) continue;
        ++acc.common;
        if (a.mult) acc.dot += a.mult[i] * a.mult[j];
        if (a.table && (uint64_t)u < (uint64_t)a.n) {
            int64_t d = a.deg_ptr[u + 1] - a.deg_ptr[u];
            d = d < 0 ? 0 : (d >= a.table_len ? a.table_len - 1 : d);
            acc.aa += a.table[d];
        }
    }
}

__device__ __forceinline__ void put_meet(const MeetArgs& a, int64_t task, const Meet& acc) {
    a.common[task] = acc.common;
    if (a.dot) a.dot[task] = a.mult ? acc.dot : acc.common;
    if (a.aa) a.aa[task] = acc.aa;
    if (a.sizes) {
        int64_t lo, hi;
        row_bounds(a, a.first[task], lo, hi);
        a.sizes[task] = hi - lo;
        row_bounds(a, a.second[task], lo, hi);
        a.sizes[a.tasks + task] = hi - lo;
    }
}

// the shorter list first
__device__ __forceinline__ void task_lists(const MeetArgs& a, int64_t task, int64_t& a0, int64_t& a1, int64_t& b0, int64_t& b1) {
    row_bounds(a, a.first[task], a0, a1);
    row_bounds(a, a.second[task], b0, b1);
    if (a1 - a0 > b1 - b0) {
        int64_t t = a0; a0 = b0; b0 = t;
        t = a1; a1 = b1; b1 = t;
    }
}

__global__ __launch_bounds__(kBlock) void k_meet_groups(MeetArgs a, int width, int64_t heavy_min) {
    const int rank = threadIdx.x & (width - 1);
    const int64_t per_block = kBlock / width;
    const int64_t mine = threadIdx.x / width;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < a.tasks; base += (int64_t)gridDim.x * per_block) {   // (uniform in the workgroup)
        const int64_t task = base + mine;
        const bool live = task < a.tasks;
        Meet acc{0, 0, 0.0};
        bool heavy = false;
        if (live) {
            int64_t a0, a1, b0, b1;
            task_lists(a, task, a0, a1, b0, b1);
            heavy = a1 - a0 >= heavy_min;
            if (!heavy) meet_lists(a, a0, a1, b0, b1, rank, width, acc);
        }
        group_sum(width, acc.common, acc.dot, acc.aa);                                  // (partners share the task: both are here)
        if (live && rank == 0) {
            if (heavy) a.heavy_list[atomicAdd(a.heavy_count, 1ull)] = task;             // (each task at most once: the list holds `tasks` entries)
            else put_meet(a, task, acc);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_meet_blocks(MeetArgs a) {
    __shared__ int64_t s_common[kWavesPerBlock], s_dot[kWavesPerBlock];
    __shared__ double s_aa[kWavesPerBlock];
    int64_t listed = (int64_t)*a.heavy_count;
    listed = listed > a.tasks ? a.tasks : listed;
    for (int64_t i = blockIdx.x; i < listed; i += gridDim.x) {
        const int64_t task = a.heavy_list[i];
        if ((uint64_t)task >= (uint64_t)a.tasks) continue;                              // (uniform in the workgroup)
        int64_t a0, a1, b0, b1;
        task_lists(a, task, a0, a1, b0, b1);
        Meet acc{0, 0, 0.0};
        meet_lists(a, a0, a1, b0, b1, (int)threadIdx.x, kBlock, acc);
        acc.common = wave_sum(acc.common);
        acc.dot = wave_sum(acc.dot);
        acc.aa = wave_sum(acc.aa);
        if (lane_id() == 0) {
            s_common[wave_id()] = acc.common;
            s_dot[wave_id()] = acc.dot;
            s_aa[wave_id()] = acc.aa;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            Meet all{0, 0, 0.0};
            for (int w = 0; w < kWavesPerBlock; ++w) {
                all.common += s_common[w];
                all.dot += s_dot[w];
                all.aa += s_aa[w];
            }
            put_meet(a, task, all);
        }
        __syncthreads();
    }
}

static int run_meet(const MeetArgs& a, int width, int64_t heavy_min, hipStream_t st) {
    PP_HIP(hipMemsetAsync(a.heavy_count, 0, sizeof(unsigned long long), st));
    if (a.tasks == 0) return PP_OK;
    k_meet_groups<<<capped_grid(a.tasks, kBlock / width), kBlock, 0, st>>>(a, width, heavy_min);
    PP_LAUNCH_CHECK();
    const unsigned blocks = capped_grid(a.tasks, 1);
    k_meet_blocks<<<blocks > 512u ? 512u : blocks, kBlock, 0, st>>>(a);                  // (reads the list's length on the device: no read-back)
    PP_LAUNCH_CHECK();
    return PP_OK;
}

// ------------------------------------------------------------------ is the stored edge list the simple structure already?
__global__ __launch_bounds__(kBlock) void k_count_unordered(const int64_t* __restrict__ edge_index, int64_t m, unsigned long long* out) {
    int64_t bad = 0;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e + 1 < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t r0 = edge_index[e], r1 = edge_index[e + 1], c0 = edge_index[m + e], c1 = edge_index[m + e + 1];
        bad += !(r0 < r1 || (r0 == r1 && c0 < c1));
    }
    bad = wave_sum(bad);
    if (lane_id() == 0 && bad) atomicAdd(out, (unsigned long long)bad);
}

// ------------------------------------------------------------------ per-node counts from the scan of the per-entry counts
__global__ __launch_bounds__(kBlock) void k_row_totals(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ scan, int64_t n,
                                                      int64_t ms, int64_t* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int64_t lo, hi;
        row_span(row_ptr, v, ms, lo, hi);
        out[v] = scan[hi] - scan[lo];
    }
}

// ------------------------------------------------------------------ the closed triads of one node, written out: a wave per entry of its row
__global__ __launch_bounds__(kBlock) void k_triad_fill(MeetArgs a, int64_t v, const int64_t* __restrict__ offset, int64_t offsets, int64_t total,
                                                      int64_t* __restrict__ out) {
    int64_t v0, v1;
    row_bounds(a, v, v0, v1);
    v1 = v1 - v0 > offsets ? v0 + offsets : v1;
    for (int64_t e = v0 + (int64_t)blockIdx.x * kWavesPerBlock + wave_id(); e < v1; e += (int64_t)gridDim.x * kWavesPerBlock) {   // (uniform in the wave)
        const int64_t x = a.col[e];
        int64_t a0, a1, b0 = v0, b1 = v1;
        row_bounds(a, x, a0, a1);
        if (a1 - a0 > b1 - b0) {
            int64_t t = a0; a0 = b0; b0 = t;
            t = a1; a1 = b1; b1 = t;
        }
        int64_t at = offset[e - v0];
        for (int64_t q = a0; q < a1; q += kWave) {
            const int64_t i = q + lane_id();
            int64_t y = -1;
            bool hit = false;
            if (i < a1) {
                y = a.col[i];
                const int64_t j = lower_bound_dev(a.col, b0, b1, y);
                hit = j < b1 && a.col[j] == y;
            }
            const unsigned long long hits = __ballot(hit);
            const int64_t slot = at + __popcll(hits & lanemask_lt());
            if (hit && slot < total) {
                out[slot] = x;
                out[total + slot] = y;
            }
            at += __popcll(hits);
        }
    }
}

// ------------------------------------------------------------------ sum over the stored edges of a[src] * b[dst]
__global__ __launch_bounds__(kBlock) void k_degree_products(const int64_t* __restrict__ edge_index, int64_t m, int64_t n,
                                                           const int32_t* __restrict__ a, const int32_t* __restrict__ b, unsigned long long* out) {
    int64_t acc = 0;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t u = edge_index[e], w = edge_index[m + e];
        if ((uint64_t)u >= (uint64_t)n || (uint64_t)w >= (uint64_t)n) continue;
        acc += (a ? (int64_t)a[u] : 1) * (int64_t)b[w];
    }
    acc = wave_sum(acc);
    if (lane_id() == 0 && acc) atomicAdd(out, (unsigned long long)acc);                 // (two's complement: exact in any order)
}

// ------------------------------------------------------------------ local clustering coefficients and the mean of their float32 roundings
constexpr int kClusterGrid = 512;

__global__ __launch_bounds__(kBlock) void k_clustering(const int64_t* __restrict__ triads, const int32_t* __restrict__ deg, int64_t n,
                                                      double* __restrict__ coeff, double* __restrict__ partial) {
    __shared__ double s_part[kWavesPerBlock];
    double acc = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const int64_t d = deg[v];
        const double c = d > 1 ? (double)triads[v] / (double)(d * (d - 1)) : 0.0;        // one correctly rounded division of two exact numbers
        if (coeff) coeff[v] = c;
        acc += (double)(float)c;
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) s_part[wave_id()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double all = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) all += s_part[w];
        partial[blockIdx.x] = all;
    }
}

__global__ void k_clustering_mean(const double* __restrict__ partial, int parts, int64_t n, double* __restrict__ mean) {
    double all = 0.0;
    for (int i = 0; i < parts; ++i) all += partial[i];                                  // in index order: the same bits on every run
    mean[0] = (double)(float)(all / (double)n);                                         // (n == 0: 0 / 0, the mean of nothing)
}

// ------------------------------------------------------------------ a similarity measure per pair from the integers above
__global__ __launch_bounds__(kBlock) void k_pair_measure(int measure, const int64_t* __restrict__ common, const int64_t* __restrict__ dot,
                                                        const double* __restrict__ aa, const int64_t* __restrict__ sizes,
                                                        const int64_t* __restrict__ norm2, const int32_t* __restrict__ indeg,
                                                        const int64_t* __restrict__ pairs, int64_t P, int64_t n, double* __restrict__ out) {
    const double nan = __builtin_nan("");
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < P; p += (int64_t)gridDim.x * kBlock) {
        double r = nan;
        if (measure == PP_PAIR_OVERLAP) {
            const int64_t least = sizes[p] < sizes[P + p] ? sizes[p] : sizes[P + p];
            if (least > 0) r = (double)common[p] / (double)least;
        } else if (measure == PP_PAIR_JACCARD) {
            const int64_t both = sizes[p] + sizes[P + p] - common[p];
            r = sizes[p] == 0 && sizes[P + p] == 0 ? 1.0 : (double)common[p] / (double)both;
        } else if (measure == PP_PAIR_ADAMIC_ADAR) {
            r = common[p] > 0 ? aa[p] : 0.0;
        } else {
            const int64_t v = pairs[p], w = pairs[P + p];
            const bool known = (uint64_t)v < (uint64_t)n && (uint64_t)w < (uint64_t)n;
            if (known) r = indeg[v] == 0 || indeg[w] == 0 ? 0.0 : (double)dot[p] / (sqrt((double)norm2[p]) * sqrt((double)norm2[P + p]));
        }
        out[p] = r;
    }
}

struct TriadWs {
    int64_t *cnt, *scan, *heavy_list;
    unsigned long long* heavy_count;
    void* scan_ws;
    size_t scan_bytes, total;
};

static TriadWs carve_triads(void* ws, int64_t tasks, bool with_scan) {
    Arena a(ws, 0);
    TriadWs w{};
    w.heavy_list = a.take<int64_t>(tasks);
    w.heavy_count = a.take<unsigned long long>(1);
    if (with_scan) {
        w.cnt = a.take<int64_t>(tasks);
        w.scan = a.take<int64_t>(tasks + 1);
        w.scan_bytes = scan_ws_bytes(tasks);
        w.scan_ws = a.take<char>((int64_t)w.scan_bytes);
    }
    w.total = a.used;
    return w;
}

}  // namespace pp

extern "C" {

int pp_graph_count_unordered(const int64_t* edge_index, int64_t m, int64_t* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(m >= 0 && out && (m == 0 || edge_index), PP_ERR_ARG, "pp_graph_count_unordered: bad argument");
    hipStream_t st = (hipStream_t)stream;
    PP_HIP(hipMemsetAsync(out, 0, sizeof(int64_t), st));
    if (m < 2) return PP_OK;
    k_count_unordered<<<capped_grid(m, kBlock), kBlock, 0, st>>>(edge_index, m, (unsigned long long*)out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_graph_meet_ws_bytes(int64_t tasks) { return pp::carve_triads(nullptr, tasks > 0 ? tasks : 0, false).total; }

int pp_graph_triad_entry_counts(const int64_t* row_ptr, const int64_t* row, const int64_t* col, int64_t n, int64_t ms, int64_t e0, int64_t e1,
                                int group, int64_t heavy_min, int64_t* cnt, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && ms >= 0 && 0 <= e0 && e0 <= e1 && e1 <= ms, PP_ERR_ARG, "pp_graph_triad_entry_counts: bad sizes");
    PP_REQUIRE(row_width_ok(group) && heavy_min >= 0, PP_ERR_ARG, "pp_graph_triad_entry_counts: group must be 0 or a power of two up to 64");
    PP_REQUIRE(e1 == e0 || (row_ptr && row && col && cnt), PP_ERR_ARG, "pp_graph_triad_entry_counts: null argument");
    PP_REQUIRE(ws_bytes >= pp_graph_meet_ws_bytes(e1 - e0), PP_ERR_WORKSPACE, "pp_graph_triad_entry_counts: workspace too small");
    const TriadWs w = carve_triads(ws, e1 - e0, false);
    MeetArgs a{};
    a.row_ptr = row_ptr; a.col = col; a.n = n; a.ms = ms;
    a.first = col + e0; a.second = row + e0; a.tasks = e1 - e0;
    a.common = cnt; a.heavy_list = w.heavy_list; a.heavy_count = w.heavy_count;
    return run_meet(a, row_width(group, n, ms), heavy_min > 0 ? heavy_min : kHeavyMinDefault, (hipStream_t)stream);
}

size_t pp_graph_triad_node_counts_ws_bytes(int64_t ms) { return pp::carve_triads(nullptr, ms > 0 ? ms : 0, true).total; }

int pp_graph_triad_node_counts(const int64_t* row_ptr, const int64_t* row, const int64_t* col, int64_t n, int64_t ms, int group, int64_t heavy_min,
                               int64_t* triads, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && ms >= 0, PP_ERR_ARG, "pp_graph_triad_node_counts: negative size");
    PP_REQUIRE(row_width_ok(group) && heavy_min >= 0, PP_ERR_ARG, "pp_graph_triad_node_counts: group must be 0 or a power of two up to 64");
    PP_REQUIRE(n == 0 || (row_ptr && triads), PP_ERR_ARG, "pp_graph_triad_node_counts: null argument");
    PP_REQUIRE(ms == 0 || (row && col), PP_ERR_ARG, "pp_graph_triad_node_counts: null argument");
    PP_REQUIRE(ws_bytes >= pp_graph_triad_node_counts_ws_bytes(ms), PP_ERR_WORKSPACE, "pp_graph_triad_node_counts: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return PP_OK;
    const TriadWs w = carve_triads(ws, ms, true);
    MeetArgs a{};
    a.row_ptr = row_ptr; a.col = col; a.n = n; a.ms = ms;
    a.first = col; a.second = row; a.tasks = ms;
    a.common = w.cnt; a.heavy_list = w.heavy_list; a.heavy_count = w.heavy_count;
    int rc = run_meet(a, row_width(group, n, ms), heavy_min > 0 ? heavy_min : kHeavyMinDefault, st);
    if (rc != PP_OK) return rc;
    rc = exclusive_scan<int64_t, int64_t>(w.cnt, ms, w.scan, true, nullptr, w.scan_ws, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    k_row_totals<<<capped_grid(n, kBlock), kBlock, 0, st>>>(row_ptr, w.scan, n, ms, triads);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_pair_meets(const int64_t* row_ptr, const int64_t* col, const int64_t* mult, int64_t n, int64_t ms, const int64_t* pairs, int64_t P,
                        const int64_t* deg_ptr, const double* table, int64_t table_len, int group, int64_t heavy_min, int64_t* common,
                        int64_t* dot, double* aa, int64_t* sizes, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && ms >= 0 && P >= 0 && table_len >= 0, PP_ERR_ARG, "pp_graph_pair_meets: negative size");
    PP_REQUIRE(row_width_ok(group) && heavy_min >= 0, PP_ERR_ARG, "pp_graph_pair_meets: group must be 0 or a power of two up to 64");
    PP_REQUIRE(P == 0 || (pairs && common && (n == 0 || row_ptr) && (ms == 0 || col)), PP_ERR_ARG, "pp_graph_pair_meets: null argument");
    PP_REQUIRE(!aa || (table && deg_ptr && table_len >= 1), PP_ERR_ARG, "pp_graph_pair_meets: aa needs the table and the stored row pointers");
    PP_REQUIRE(ws_bytes >= pp_graph_meet_ws_bytes(P), PP_ERR_WORKSPACE, "pp_graph_pair_meets: workspace too small");
    const TriadWs w = carve_triads(ws, P, false);
    MeetArgs a{};
    a.row_ptr = row_ptr; a.col = col; a.mult = mult; a.n = n; a.ms = ms;
    a.first = pairs; a.second = pairs + P; a.tasks = P;
    a.deg_ptr = deg_ptr; a.table = aa ? table : nullptr; a.table_len = table_len;
    a.common = common; a.dot = dot; a.aa = aa; a.sizes = sizes;
    a.heavy_list = w.heavy_list; a.heavy_count = w.heavy_count;
    return run_meet(a, row_width(group, n, ms), heavy_min > 0 ? heavy_min : kHeavyMinDefault, (hipStream_t)stream);
}

int pp_pair_measure(int measure, const int64_t* common, const int64_t* dot, const double* aa, const int64_t* sizes, const int64_t* norm2,
                    const int32_t* indeg, const int64_t* pairs, int64_t P, int64_t n, double* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(P >= 0 && n >= 0, PP_ERR_ARG, "pp_pair_measure: negative size");
    PP_REQUIRE(measure >= PP_PAIR_OVERLAP && measure <= PP_PAIR_COSINE, PP_ERR_ARG, "pp_pair_measure: unknown measure %d", measure);
    if (P == 0) return PP_OK;
    PP_REQUIRE(common && out, PP_ERR_ARG, "pp_pair_measure: null argument");
    PP_REQUIRE((measure != PP_PAIR_OVERLAP && measure != PP_PAIR_JACCARD) || sizes, PP_ERR_ARG, "pp_pair_measure: the list lengths are required");
    PP_REQUIRE(measure != PP_PAIR_ADAMIC_ADAR || aa, PP_ERR_ARG, "pp_pair_measure: aa is required");
    PP_REQUIRE(measure != PP_PAIR_COSINE || (dot && norm2 && indeg && pairs), PP_ERR_ARG, "pp_pair_measure: cosine needs dot, norm2, indeg and pairs");
    k_pair_measure<<<capped_grid(P, kBlock), kBlock, 0, (hipStream_t)stream>>>(measure, common, dot, aa, sizes, norm2, indeg, pairs, P, n, out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_triad_fill(const int64_t* row_ptr, const int64_t* col, int64_t n, int64_t ms, int64_t v, const int64_t* offset, int64_t offsets,
                        int64_t total, int64_t* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && ms >= 0 && total >= 0 && offsets >= 0, PP_ERR_ARG, "pp_graph_triad_fill: negative size");
    PP_REQUIRE(v >= 0 && v < n, PP_ERR_ARG, "pp_graph_triad_fill: node index out of range");
    PP_REQUIRE(row_ptr && (ms == 0 || col) && (total == 0 || (offset && out)), PP_ERR_ARG, "pp_graph_triad_fill: null argument");
    if (total == 0 || ms == 0) return PP_OK;
    MeetArgs a{};
    a.row_ptr = row_ptr; a.col = col; a.n = n; a.ms = ms;
    k_triad_fill<<<capped_grid(ms, kWavesPerBlock), kBlock, 0, (hipStream_t)stream>>>(a, v, offset, offsets, total, out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_degree_product_sum(const int64_t* edge_index, int64_t m, int64_t n, const int32_t* a, const int32_t* b, int64_t* out, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(m >= 0 && n >= 0 && out && (m == 0 || (edge_index && b)), PP_ERR_ARG, "pp_degree_product_sum: bad argument");
    hipStream_t st = (hipStream_t)stream;
    PP_HIP(hipMemsetAsync(out, 0, sizeof(int64_t), st));
    if (m == 0) return PP_OK;
    k_degree_products<<<capped_grid(m, kBlock), kBlock, 0, st>>>(edge_index, m, n, a, b, (unsigned long long*)out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_graph_clustering_ws_bytes(void) { return pp::align_up((size_t)pp::kClusterGrid * sizeof(double)); }

int pp_graph_clustering(const int64_t* triads, const int32_t* deg, int64_t n, double* coeff, double* mean, void* ws, size_t ws_bytes,
                        pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && (n == 0 || (triads && deg)) && (coeff || mean), PP_ERR_ARG, "pp_graph_clustering: bad argument");
    PP_REQUIRE(ws_bytes >= pp_graph_clustering_ws_bytes(), PP_ERR_WORKSPACE, "pp_graph_clustering: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int64_t g = ceil_div(n > 0 ? n : 1, kBlock);
    const int parts = (int)(g > kClusterGrid ? kClusterGrid : g);
    k_clustering<<<parts, kBlock, 0, st>>>(triads, deg, n, coeff, (double*)ws);
    PP_LAUNCH_CHECK();
    if (mean) {
        k_clustering_mean<<<1, 1, 0, st>>>((const double*)ws, parts, n, mean);
        PP_LAUNCH_CHECK();
    }
    return PP_OK;
}

}  // extern "C"
