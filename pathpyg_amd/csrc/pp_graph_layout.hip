// pathpyg_amd — node layouts of a static Graph: Fruchterman-Reingold ("spring"), random, circular, grid.
//
// Reference: src/pathpyG/visualisations/layout.py:69-269 hands the spring names to networkx.spring_layout, whose dense routine runs, per
// iteration, an all-pairs force sum in numpy (float64, O(n^2) memory and time).  Here the same iteration, float64 throughout, at every n:
//   disp_i = sum_j (p_i - p_j) (k^2 / max(d_ij, 0.01)^2 - A_ij max(d_ij, 0.01) / k);  len_i = |disp_i|, 0.1 where that is < 0.01;
//   p_i += disp_i (t / len_i) unless i is fixed;  t -= dt;  stop after the first iteration with sqrt(sum |dp_i|^2) / n < threshold.
// Launches of one iteration, all plain, on one stream; no cooperative launch, no grid barrier, no floating-point atomic:
//   1. k_layout_repulse, grid (target blocks, source chunks): a workgroup owns `block` target nodes (one per thread) and one chunk of the
//      source range.  It walks the chunk in tiles of kLayoutTile positions staged in LDS (16 bytes per node; every lane reads the same
//      word, a broadcast).  Per pair: one reciprocal of max(d^2, 0.01^2), no square root; four accumulators per axis (source j of the chunk
//      goes to accumulator j mod 4), folded (0 + 1) + (2 + 3).  The pair i == j adds an exact 0.  Output: part[chunk][i], a fixed shape.
//   2. k_layout_attract_groups: a node belongs to a GROUP of `width` lanes; lane s adds the CSR entries s, s + width, ... of the node in
//      order, the lanes fold by a butterfly.  Lane 0 of the group then finishes the node: it adds part[0][i], part[1][i], ... in order,
//      forms disp = k^2 rep - att / k, applies the length rule, the step and the fixed mask, writes the new position to the OTHER buffer
//      and adds |dp|^2 to the workgroup's partial.  A node of heavy_min entries or more is left to
//   3. k_layout_attract_blocks (only if there are such nodes): a whole workgroup per node, thread j adds entries j, j + 256, ... .
//   4. k_layout_decide (one workgroup): folds the partials of sum |dp|^2, counts the iteration, swaps the buffers, cools t and sets `done`
//      if the criterion holds (written `err < threshold`: a NaN does not stop the run, as in numpy).
// Every kernel reads state[done] first and returns once it is set: the iterate that first met the criterion stays where it is.  The host
// enqueues a batch of iterations, synchronises once and reads the state words.
// Determinism: the order of the adds of a node depends on n, `chunks`, `width` and heavy_min only — never on the grid, on which workgroup
// runs first or on the batch.  Partials are folded by index in a fixed shape.  The list of heavy nodes is built by a scan, ascending.
//
// The adjacency is what the reference builds through scipy and networkx: one entry per unordered pair with a stored edge in either direction,
// its value the weight of the LAST such edge in stored order, self-loops dropped.  Both directions of every stored edge become an entry
// keyed row * n + col; a stable sort groups the copies of an entry in stored order, the last of a run wins, a scan compacts the winners —
// sorted by (row, col), which is the CSR.
#include "pp_common.h"
#include "pp_internal.h"
#include "pp_philox.h"
#include "pp_rows.h"

namespace pp {

constexpr int kLayoutTile = 256;                       // source positions staged per round: 4 KiB of LDS
constexpr int64_t kLayoutBatch = 16;
constexpr int64_t kLayoutMaxChunks = 64;
constexpr int64_t kLayoutFillGrid = 2048;              // workgroups the repulsion grid aims at: 256 CUs x 8 resident workgroups
constexpr int64_t kLayoutLightParts = kMaxGrid - kBlock, kLayoutHeavyParts = kBlock;
enum { kLT = kStateShared, kLDt = 5, kLErr = 6, kLStateWords = 8 };   // after the shared words of pp_rows.h; words 4 .. 6 hold doubles

static bool layout_block_ok(int block) { return block == 0 || block == 64 || block == 128 || block == 256; }
static int64_t layout_chunks(int64_t n, int block, int64_t chunks) {
    if (chunks > 0) return chunks;
    const int64_t targets = ceil_div(n > 0 ? n : 1, block > 0 ? block : kBlock), tiles = ceil_div(n > 0 ? n : 1, kLayoutTile);
    int64_t c = ceil_div(kLayoutFillGrid, targets);
    c = c > tiles ? tiles : c;
    return c > kLayoutMaxChunks ? kLayoutMaxChunks : (c < 1 ? 1 : c);
}

struct LayoutArgs {
    const int64_t* ptr;            // [n + 1]
    const int64_t* nbr;            // [nnz]
    const double* w;               // [nnz] or nullptr: every entry 1
    const uint8_t* fixed;          // [n] or nullptr
    int64_t n, nnz, heavy_min, chunks, chunk_len;
    double k, threshold;
    double2 *p0, *p1;              // the positions: state[kCur] says which is current
    double2* part;                 // [chunks][n] repulsion sums
    double* err_part;              // light workgroups first, heavy ones from `light_parts` on
    int64_t light_parts, heavy_parts;
    const int32_t* heavy_list;     // ascending
    int64_t* state;                // kLStateWords
};

__device__ __forceinline__ double2* layout_buffer(const LayoutArgs& a, int which) { return which ? a.p1 : a.p0; }
__device__ __forceinline__ double layout_state_f(const LayoutArgs& a, int word) { return __longlong_as_double(a.state[word]); }

// ------------------------------------------------------------------ the iteration
__device__ __forceinline__ void layout_pair(double2 pi, double2 pj, double& sx, double& sy) {
    const double dx = pi.x - pj.x, dy = pi.y - pj.y, d2 = dx * dx + dy * dy;
    const double inv = 1.0 / (d2 < 0.01 * 0.01 ? 0.01 * 0.01 : d2);                     // (a NaN stays a NaN, as under numpy's clip)
    sx += dx * inv;
    sy += dy * inv;
}

__global__ __launch_bounds__(kBlock) void k_layout_repulse(LayoutArgs a) {
    __shared__ double2 tile[kLayoutTile];
    if (a.state[kDone]) return;                                                        // (uniform in the grid)
    const double2* p = layout_buffer(a, (int)(a.state[kCur] & 1));
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < a.n;
    const double2 pi = live ? p[i] : make_double2(0.0, 0.0);
    const int64_t lo = (int64_t)blockIdx.y * a.chunk_len;
    int64_t hi = lo + a.chunk_len;
    hi = hi > a.n ? a.n : hi;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
    for (int64_t base = lo; base < hi; base += kLayoutTile) {                           // (uniform in the workgroup)
        const int count = (int)(hi - base < kLayoutTile ? hi - base : kLayoutTile);
        __syncthreads();
        for (int s = threadIdx.x; s < count; s += blockDim.x) tile[s] = p[base + s];
        __syncthreads();
        if (!live) continue;
        int j = 0;
        for (; j + 4 <= count; j += 4) {
            layout_pair(pi, tile[j], x0, y0);
            layout_pair(pi, tile[j + 1], x1, y1);
            layout_pair(pi, tile[j + 2], x2, y2);
            layout_pair(pi, tile[j + 3], x3, y3);
        }
        if (j < count) layout_pair(pi, tile[j], x0, y0);                                // (kLayoutTile % 4 == 0: j mod 4 is the chunk's)
        if (j + 1 < count) layout_pair(pi, tile[j + 1], x1, y1);
        if (j + 2 < count) layout_pair(pi, tile[j + 2], x2, y2);
    }
    if (live) a.part[(int64_t)blockIdx.y * a.n + i] = make_double2((x0 + x1) + (x2 + x3), (y0 + y1) + (y2 + y3));
}

// entries lo + sub, lo + sub + step, ... of one neighbour list, added in that order: sum_u w (p_v - p_u) max(d, 0.01)
__device__ __forceinline__ double2 layout_row_sum(const LayoutArgs& a, const double2* __restrict__ p, double2 pv, int64_t lo, int64_t hi, int sub,
                                                   int step) {
    double sx = 0.0, sy = 0.0;
    for (int64_t e = lo + sub; e < hi; e += step) {
        const int64_t u = load_stream(a.nbr + e);
        if ((uint64_t)u >= (uint64_t)a.n) continue;
        const double2 pu = p[u];
        const double dx = pv.x - pu.x, dy = pv.y - pu.y;
        double d = sqrt(dx * dx + dy * dy);
        d = d < 0.01 ? 0.01 : d;
        const double f = a.w ? load_stream(a.w + e) * d : d;
        sx += dx * f;
        sy += dy * f;
    }
    return make_double2(sx, sy);
}

// the new position of node v from its attraction sum; returns |dp|^2
__device__ __forceinline__ double layout_finish(const LayoutArgs& a, double2* __restrict__ out, int64_t v, double2 pv, double2 att, double t) {
    double rx = 0.0, ry = 0.0;
    for (int64_t c = 0; c < a.chunks; ++c) {
        const double2 r = a.part[c * a.n + v];
        rx += r.x;
        ry += r.y;
    }
    const double k2 = a.k * a.k, dx = k2 * rx - att.x / a.k, dy = k2 * ry - att.y / a.k;
    double len = sqrt(dx * dx + dy * dy);
    if (len < 0.01) len = 0.1;
    const double f = t / len;
    double sx = dx * f, sy = dy * f;
    if (a.fixed && a.fixed[v]) sx = sy = 0.0;
    out[v] = make_double2(pv.x + sx, pv.y + sy);
    return sx * sx + sy * sy;
}

__global__ __launch_bounds__(kBlock) void k_layout_attract_groups(LayoutArgs a, int width) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;
    const int cur = (int)(a.state[kCur] & 1);
    const double2* p = layout_buffer(a, cur);
    double2* out = layout_buffer(a, cur ^ 1);
    const double t = layout_state_f(a, kLT);
    const int sub = threadIdx.x & (width - 1);
    const int64_t per_block = kBlock / width, mine = threadIdx.x / width;
    double err = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < a.n; base += (int64_t)gridDim.x * per_block) {       // (uniform in the workgroup)
        const int64_t v = base + mine;
        const bool live = v < a.n;
        bool heavy = false;
        double2 pv = make_double2(0.0, 0.0), s = make_double2(0.0, 0.0);
        if (live) {
            int64_t lo, hi;
            row_span(a.ptr, v, a.nnz, lo, hi);
            heavy = hi - lo >= a.heavy_min;
            pv = p[v];
            if (!heavy) s = layout_row_sum(a, p, pv, lo, hi, sub, width);
        }
        group_sum(width, s.x, s.y);                                                     // (partners share the node: both are here)
        if (live && sub == 0 && !heavy) err += layout_finish(a, out, v, pv, s, t);
    }
    err = block_sum_fixed(err, scratch);
    if (threadIdx.x == 0) a.err_part[blockIdx.x] = err;
}

__global__ __launch_bounds__(kBlock) void k_layout_attract_blocks(LayoutArgs a) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;
    const int cur = (int)(a.state[kCur] & 1);
    const double2* p = layout_buffer(a, cur);
    double2* out = layout_buffer(a, cur ^ 1);
    const double t = layout_state_f(a, kLT);
    const int64_t heavy_count = a.state[kHeavyCount];
    double err = 0.0;                                                                   // (thread 0's is the workgroup's)
    for (int64_t i = blockIdx.x; i < heavy_count; i += gridDim.x) {
        const int64_t v = a.heavy_list[i];
        if ((uint64_t)v >= (uint64_t)a.n) continue;                                     // (uniform in the workgroup)
        int64_t lo, hi;
        row_span(a.ptr, v, a.nnz, lo, hi);
        const double2 pv = p[v];
        double2 s = layout_row_sum(a, p, pv, lo, hi, (int)threadIdx.x, kBlock);
        s.x = block_sum_fixed(s.x, scratch);
        s.y = block_sum_fixed(s.y, scratch);
        if (threadIdx.x == 0) err += layout_finish(a, out, v, pv, s, t);
    }
    if (threadIdx.x == 0) a.err_part[a.light_parts + blockIdx.x] = err;
}

__global__ __launch_bounds__(kBlock) void k_layout_decide(LayoutArgs a) {
    __shared__ double scratch[kWavesPerBlock];
    if (a.state[kDone]) return;
    const double total = fold_parts(a.err_part, a.light_parts + a.heavy_parts, scratch);
    if (threadIdx.x == 0) {
        const double err = sqrt(total) / (double)a.n;
        a.state[kIters] += 1;
        a.state[kCur] ^= 1;
        a.state[kLT] = __double_as_longlong(layout_state_f(a, kLT) - layout_state_f(a, kLDt));
        a.state[kLErr] = __double_as_longlong(err);
        if (err < a.threshold) a.state[kDone] = 1;                                     // (false for a NaN)
    }
}

// ------------------------------------------------------------------ set-up and result
// per workgroup: {min x, max x, min y, max y} of its positions (a workgroup without a position writes the first node's)
__global__ __launch_bounds__(kBlock) void k_layout_extent_parts(const double2* __restrict__ p, int64_t n, double* __restrict__ part) {
    __shared__ double scratch[kWavesPerBlock];
    const double2 first = p[0];
    double lx = first.x, hx = first.x, ly = first.y, hy = first.y;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const double2 q = p[v];
        lx = q.x < lx ? q.x : lx; hx = q.x > hx ? q.x : hx;
        ly = q.y < ly ? q.y : ly; hy = q.y > hy ? q.y : hy;
    }
    lx = -block_max_fixed(-lx, scratch); hx = block_max_fixed(hx, scratch);
    ly = -block_max_fixed(-ly, scratch); hy = block_max_fixed(hy, scratch);
    if (threadIdx.x == 0) { part[4 * blockIdx.x] = lx; part[4 * blockIdx.x + 1] = hx; part[4 * blockIdx.x + 2] = ly; part[4 * blockIdx.x + 3] = hy; }
}

// t = 0.1 max(extent x, extent y), dt = t / (iterations + 1)
__global__ __launch_bounds__(kBlock) void k_layout_temperature(const double* __restrict__ part, int64_t parts, int64_t iterations, int64_t* state) {
    __shared__ double scratch[kWavesPerBlock];
    double lx = part[0], hx = part[1], ly = part[2], hy = part[3];
    for (int64_t i = threadIdx.x; i < parts; i += kBlock) {
        lx = part[4 * i] < lx ? part[4 * i] : lx; hx = part[4 * i + 1] > hx ? part[4 * i + 1] : hx;
        ly = part[4 * i + 2] < ly ? part[4 * i + 2] : ly; hy = part[4 * i + 3] > hy ? part[4 * i + 3] : hy;
    }
    lx = -block_max_fixed(-lx, scratch); hx = block_max_fixed(hx, scratch);
    ly = -block_max_fixed(-ly, scratch); hy = block_max_fixed(hy, scratch);
    if (threadIdx.x == 0) {
        const double ex = hx - lx, ey = hy - ly, t = (ex > ey ? ex : ey) * 0.1;
        state[kLT] = __double_as_longlong(t);
        state[kLDt] = __double_as_longlong(t / (double)(iterations + 1));
    }
}

__global__ __launch_bounds__(kBlock) void k_layout_copy(const double2* __restrict__ src, int64_t n, double2* __restrict__ dst) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) dst[v] = src[v];
}

__global__ __launch_bounds__(kBlock) void k_layout_result(const LayoutArgs a, double2* __restrict__ pos) {
    const double2* p = layout_buffer(a, (int)(a.state[kCur] & 1));
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) pos[v] = p[v];
}

struct LayoutWs {
    int64_t* state;
    double *err_part, *extent_part;
    double2 *p0, *p1, *part;
    int32_t *flag, *pos, *heavy_list;
    void* scan;
    size_t scan_bytes, total;
};

static LayoutWs carve_layout(void* ws, int64_t n, int64_t chunks) {
    Arena a(ws, 0);
    LayoutWs w{};
    w.state = a.take<int64_t>(kLStateWords);
    w.err_part = a.take<double>(kMaxGrid);
    w.extent_part = a.take<double>(4 * kMaxGrid);
    w.p0 = a.take<double2>(n);
    w.p1 = a.take<double2>(n);
    w.part = a.take<double2>(n * chunks);
    w.flag = a.take<int32_t>(n);
    w.pos = a.take<int32_t>(n + 1);
    w.heavy_list = a.take<int32_t>(n);
    w.scan_bytes = scan_ws_bytes(n);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.total = a.used;
    return w;
}

// ------------------------------------------------------------------ rescale (networkx.rescale_layout, then + center)
__global__ __launch_bounds__(kBlock) void k_layout_sum_parts(const double2* __restrict__ p, int64_t n, double* __restrict__ part) {
    __shared__ double scratch[kWavesPerBlock];
    double sx = 0.0, sy = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) { sx += p[v].x; sy += p[v].y; }
    sx = block_sum_fixed(sx, scratch);
    sy = block_sum_fixed(sy, scratch);
    if (threadIdx.x == 0) { part[blockIdx.x] = sx; part[gridDim.x + blockIdx.x] = sy; }
}

// p -= mean (every workgroup folds the same partials in the same shape: all hold the same mean); one partial of max |p| per workgroup
__global__ __launch_bounds__(kBlock) void k_layout_center(double2* __restrict__ p, int64_t n, const double* part, double* __restrict__ lim_part) {
    __shared__ double scratch[kWavesPerBlock];
    const double mx = fold_parts(part, gridDim.x, scratch) / (double)n, my = fold_parts(part + gridDim.x, gridDim.x, scratch) / (double)n;
    double lim = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const double2 q = make_double2(p[v].x - mx, p[v].y - my);
        p[v] = q;
        const double m = fabs(q.x) > fabs(q.y) ? fabs(q.x) : fabs(q.y);
        lim = m > lim ? m : lim;
    }
    lim = block_max_fixed(lim, scratch);
    if (threadIdx.x == 0) lim_part[blockIdx.x] = lim;
}

__global__ __launch_bounds__(kBlock) void k_layout_scale(double2* __restrict__ p, int64_t n, const double* lim_part, double scale, double cx, double cy) {
    __shared__ double scratch[kWavesPerBlock];
    double lim = 0.0;
    for (int64_t i = threadIdx.x; i < gridDim.x; i += kBlock) lim = lim_part[i] > lim ? lim_part[i] : lim;
    lim = block_max_fixed(lim, scratch);
    const double f = lim > 0.0 ? scale / lim : 1.0;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
        p[v] = make_double2(p[v].x * f + cx, p[v].y * f + cy);
}

// ------------------------------------------------------------------ draws and the closed-form layouts
__device__ __forceinline__ double layout_uniform(uint32_t k0, uint32_t k1, uint64_t index) {        // 53 bits, [0, 1)
    return (double)(rg_word(k0, k1, PP_RG_TAG_LAYOUT, 0, index) >> 11) * 0x1p-53;
}

__global__ __launch_bounds__(kBlock) void k_layout_start(uint32_t k0, uint32_t k1, int64_t n, double dom_size, double cx, double cy,
                                                        const double2* __restrict__ given, const uint8_t* __restrict__ has, double2* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        if (given && (!has || has[v])) { out[v] = given[v]; continue; }
        out[v] = make_double2(layout_uniform(k0, k1, 2 * (uint64_t)v) * dom_size + cx, layout_uniform(k0, k1, 2 * (uint64_t)v + 1) * dom_size + cy);
    }
}

__global__ __launch_bounds__(kBlock) void k_layout_random_f32(uint32_t k0, uint32_t k1, int64_t n, float cx, float cy, float2* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        const float x = (float)(rg_word(k0, k1, PP_RG_TAG_LAYOUT, 0, 2 * (uint64_t)v) >> 40) * 0x1p-24f;          // 24 bits: exact in float32
        const float y = (float)(rg_word(k0, k1, PP_RG_TAG_LAYOUT, 0, 2 * (uint64_t)v + 1) >> 40) * 0x1p-24f;
        out[v] = make_float2(x + cx, y + cy);
    }
}

__global__ __launch_bounds__(kBlock) void k_layout_closed_form(int kind, int64_t n, double2* __restrict__ out) {
    const double side = floor(sqrt((double)n)), dist = 1.0 / side;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        if (kind == PP_LAYOUT_CIRCULAR) {                                               // networkx: the angle in float32, then cos and sin
            const float theta = (float)((double)v * (1.0 / (double)n) * 2.0 * 3.141592653589793);
            out[v] = make_double2((double)cosf(theta), (double)sinf(theta));
        } else {                                                                        // the reference's grid (layout.py:258-269)
            const double col = fmod((double)v, side), row = floor((double)v / side);
            out[v] = make_double2(col * dist, -row * dist);
        }
    }
}

// ------------------------------------------------------------------ the adjacency
__global__ __launch_bounds__(kBlock) void k_layout_adj_keys(const int64_t* __restrict__ ei, int64_t m, int64_t n, uint64_t* __restrict__ key) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t u = ei[e], v = ei[m + e];
        const bool keep = (uint64_t)u < (uint64_t)n && (uint64_t)v < (uint64_t)n && u != v;
        const uint64_t none = (uint64_t)n * (uint64_t)n;                                // (sorts behind every entry)
        key[2 * e] = keep ? (uint64_t)u * (uint64_t)n + (uint64_t)v : none;
        key[2 * e + 1] = keep ? (uint64_t)v * (uint64_t)n + (uint64_t)u : none;
    }
}

__global__ __launch_bounds__(kBlock) void k_layout_adj_flags(const uint64_t* __restrict__ sorted, int64_t count, int64_t n, int32_t* __restrict__ flag) {
    const uint64_t none = (uint64_t)n * (uint64_t)n;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock)
        flag[i] = sorted[i] != none && (i + 1 == count || sorted[i + 1] != sorted[i]);  // the last copy in stored order
}

__global__ __launch_bounds__(kBlock) void k_layout_adj_fill(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ entry,
                                                           const int32_t* __restrict__ flag, const int64_t* __restrict__ pos, int64_t count, int64_t n,
                                                           int64_t m, int64_t nnz, const double* __restrict__ weight, int64_t* __restrict__ row,
                                                           int64_t* __restrict__ nbr, double* __restrict__ w) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        if (!flag[i]) continue;
        const int64_t o = pos[i], e = (int64_t)(entry[i] >> 1);
        if ((uint64_t)o >= (uint64_t)nnz || e >= m) continue;
        row[o] = (int64_t)(sorted[i] / (uint64_t)n);
        nbr[o] = (int64_t)(sorted[i] % (uint64_t)n);
        w[o] = weight ? weight[e] : 1.0;
    }
}

// ptr[r] = the first entry whose row is >= r; the entries are sorted by row (every word of ptr has one writer)
__global__ __launch_bounds__(kBlock) void k_layout_adj_ptr(const int64_t* __restrict__ row, int64_t nnz, int64_t n, int64_t* __restrict__ ptr) {
    for (int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x; o < nnz; o += (int64_t)gridDim.x * kBlock) {
        int64_t r = row[o], before = o > 0 ? row[o - 1] : -1;
        r = r < 0 ? 0 : (r >= n ? n - 1 : r);
        before = before < -1 ? -1 : (before >= n ? n - 1 : before);
        for (int64_t x = before + 1; x <= r; ++x) ptr[x] = o;
        if (o + 1 == nnz) for (int64_t x = r + 1; x <= n; ++x) ptr[x] = nnz;
    }
}

struct LayoutAdjWs {
    int64_t* total;
    uint64_t *key, *sorted;
    uint32_t* entry;
    int32_t* flag;
    int64_t *pos, *row;
    void *sort, *scan;
    size_t sort_bytes, scan_bytes, bytes;
};

static LayoutAdjWs carve_layout_adj(void* ws, int64_t m) {
    Arena a(ws, 0);
    LayoutAdjWs w{};
    const int64_t count = 2 * m;
    w.total = a.take<int64_t>(2);
    w.key = a.take<uint64_t>(count);
    w.sorted = a.take<uint64_t>(count);
    w.entry = a.take<uint32_t>(count);
    w.flag = a.take<int32_t>(count);
    w.pos = a.take<int64_t>(count + 1);
    w.row = a.take<int64_t>(count);
    w.sort_bytes = sort_ws_bytes(count, sizeof(uint64_t));
    w.sort = a.take<char>((int64_t)w.sort_bytes);
    w.scan_bytes = scan_ws_bytes(count);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.bytes = a.used;
    return w;
}

}  // namespace pp

extern "C" {

int64_t pp_graph_layout_heavy_min(void) { return pp::kHeavyMinDefault; }

int64_t pp_graph_layout_chunks(int64_t n, int block, int64_t chunks) { return pp::layout_chunks(n, block, chunks); }

size_t pp_graph_layout_ws_bytes(int64_t n, int block, int64_t chunks) {
    return pp::carve_layout(nullptr, n > 0 ? n : 0, pp::layout_chunks(n, block, chunks)).total;
}

int pp_graph_layout_iterate(const int64_t* ptr, const int64_t* nbr, const double* w, int64_t n, int64_t nnz, double* pos, const uint8_t* fixed,
                            double k, double t, double dt, int auto_t, int64_t iterations, double threshold, int64_t batch, int block,
                            int64_t chunks, int group, int64_t heavy_min, int64_t* iterations_run, double* last_err, int64_t* grids, void* ws,
                            size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && nnz >= 0, PP_ERR_ARG, "pp_graph_layout_iterate: negative size");
    PP_REQUIRE(n < (int64_t)0x7fffffff && nnz < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_iterate: size >= 2^31 - 1");
    PP_REQUIRE(iterations_run && last_err && grids, PP_ERR_ARG, "pp_graph_layout_iterate: iterations_run, last_err and grids are required");
    PP_REQUIRE(iterations >= 0 && batch >= 0, PP_ERR_ARG, "pp_graph_layout_iterate: iterations and batch must be >= 0");
    PP_REQUIRE(layout_block_ok(block), PP_ERR_ARG, "pp_graph_layout_iterate: block must be 0, 64, 128 or 256");
    PP_REQUIRE(chunks >= 0 && chunks <= kLayoutMaxChunks, PP_ERR_ARG, "pp_graph_layout_iterate: chunks must be 0 .. %lld", (long long)kLayoutMaxChunks);
    PP_REQUIRE(row_width_ok(group) && heavy_min >= 0, PP_ERR_ARG, "pp_graph_layout_iterate: group must be 0 or a power of two up to 64");
    PP_REQUIRE(n == 0 || (pos && ptr), PP_ERR_ARG, "pp_graph_layout_iterate: pos and ptr are required");
    PP_REQUIRE(nnz == 0 || nbr, PP_ERR_ARG, "pp_graph_layout_iterate: nbr is required");
    PP_REQUIRE(ws_bytes >= pp_graph_layout_ws_bytes(n, block, chunks), PP_ERR_WORKSPACE, "pp_graph_layout_iterate: workspace too small");
    *iterations_run = 0;
    *last_err = 0.0;
    grids[0] = grids[1] = grids[2] = grids[3] = 0;
    if (n == 0) return PP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int threads = block > 0 ? block : kBlock;
    const int64_t n_chunks = layout_chunks(n, block, chunks);
    const LayoutWs s = carve_layout(ws, n, n_chunks);
    const int width = row_width(group, n, nnz);
    const unsigned gn = capped_grid(n, kBlock, kLayoutLightParts);
    int64_t host[kLStateWords] = {0};

    LayoutArgs a{};
    a.ptr = ptr; a.nbr = nbr; a.w = w; a.fixed = fixed; a.n = n; a.nnz = nnz;
    a.heavy_min = heavy_min > 0 ? heavy_min : kHeavyMinDefault;
    a.chunks = n_chunks;
    a.chunk_len = ceil_div(n, n_chunks);
    a.k = k; a.threshold = threshold;
    a.p0 = s.p0; a.p1 = s.p1; a.part = s.part; a.err_part = s.err_part; a.heavy_list = s.heavy_list; a.state = s.state;

    // set-up: the heavy nodes (ascending, by a scan), the start positions, the temperature; one read-back
    __builtin_memcpy(&host[kLT], &t, sizeof(double));
    __builtin_memcpy(&host[kLDt], &dt, sizeof(double));
    PP_HIP(hipMemcpyAsync(s.state, host, kLStateWords * sizeof(int64_t), hipMemcpyHostToDevice, st));
    int rc = heavy_rows_ascending(ptr, n, nnz, a.heavy_min, s.flag, s.pos, s.heavy_list, s.state + kHeavyCount, s.scan, s.scan_bytes, st);
    if (rc != PP_OK) return rc;
    k_layout_copy<<<gn, kBlock, 0, st>>>((const double2*)pos, n, s.p0);
    PP_LAUNCH_CHECK();
    if (auto_t) {
        k_layout_extent_parts<<<gn, kBlock, 0, st>>>(s.p0, n, s.extent_part);
        PP_LAUNCH_CHECK();
        k_layout_temperature<<<1, kBlock, 0, st>>>(s.extent_part, (int64_t)gn, iterations, s.state);
        PP_LAUNCH_CHECK();
    }
    PP_HIP(hipMemcpyAsync(host, s.state, kLStateWords * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    const int64_t heavy_count = host[kHeavyCount] < 0 ? 0 : (host[kHeavyCount] > n ? n : host[kHeavyCount]);

    const dim3 g_repulse((unsigned)ceil_div(n, threads), (unsigned)n_chunks);
    const unsigned g_light = capped_grid(n, kBlock / width, kLayoutLightParts);
    const unsigned g_heavy = heavy_count > 0 ? capped_grid(heavy_count, 1, kLayoutHeavyParts) : 0;
    a.light_parts = g_light;
    a.heavy_parts = g_heavy;
    grids[0] = g_repulse.x; grids[1] = g_repulse.y; grids[2] = g_light; grids[3] = g_heavy;

    rc = run_batched(iterations, batch > 0 ? batch : kLayoutBatch, s.state, host, kLStateWords, st, [&]() -> int {
        k_layout_repulse<<<g_repulse, threads, 0, st>>>(a);
        PP_LAUNCH_CHECK();
        k_layout_attract_groups<<<g_light, kBlock, 0, st>>>(a, width);
        PP_LAUNCH_CHECK();
        if (g_heavy > 0) {
            k_layout_attract_blocks<<<g_heavy, kBlock, 0, st>>>(a);
            PP_LAUNCH_CHECK();
        }
        k_layout_decide<<<1, kBlock, 0, st>>>(a);
        PP_LAUNCH_CHECK();
        return PP_OK;
    });
    if (rc != PP_OK) return rc;
    *iterations_run = host[kIters];
    __builtin_memcpy(last_err, &host[kLErr], sizeof(double));
    k_layout_result<<<gn, kBlock, 0, st>>>(a, (double2*)pos);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_graph_layout_rescale_ws_bytes(void) { return pp::align_up(3 * (size_t)pp::kMaxGrid * sizeof(double)); }

int pp_graph_layout_rescale(double* pos, int64_t n, double scale, double cx, double cy, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_rescale: n outside [0, 2^31 - 1)");
    PP_REQUIRE(ws_bytes >= pp_graph_layout_rescale_ws_bytes(), PP_ERR_WORKSPACE, "pp_graph_layout_rescale: workspace too small");
    if (n == 0) return PP_OK;
    PP_REQUIRE(pos && ws, PP_ERR_ARG, "pp_graph_layout_rescale: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned g = capped_grid(n, kBlock);
    double* part = (double*)ws;
    k_layout_sum_parts<<<g, kBlock, 0, st>>>((const double2*)pos, n, part);
    PP_LAUNCH_CHECK();
    k_layout_center<<<g, kBlock, 0, st>>>((double2*)pos, n, part, part + 2 * kMaxGrid);
    PP_LAUNCH_CHECK();
    k_layout_scale<<<g, kBlock, 0, st>>>((double2*)pos, n, part + 2 * kMaxGrid, scale, cx, cy);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_layout_start(int64_t seed, int64_t n, double dom_size, double cx, double cy, const double* given, const uint8_t* has, double* pos,
                          pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_start: n outside [0, 2^31 - 1)");
    if (n == 0) return PP_OK;
    PP_REQUIRE(pos && (given || !has), PP_ERR_ARG, "pp_graph_layout_start: null pointer");
    k_layout_start<<<capped_grid(n, kBlock), kBlock, 0, (hipStream_t)stream>>>((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), n, dom_size, cx,
                                                                               cy, (const double2*)given, has, (double2*)pos);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_layout_random(int64_t seed, int64_t n, float cx, float cy, float* pos, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_random: n outside [0, 2^31 - 1)");
    if (n == 0) return PP_OK;
    PP_REQUIRE(pos, PP_ERR_ARG, "pp_graph_layout_random: null pointer");
    k_layout_random_f32<<<capped_grid(n, kBlock), kBlock, 0, (hipStream_t)stream>>>((uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), n, cx, cy,
                                                                                    (float2*)pos);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_layout_closed_form(int kind, int64_t n, double* pos, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(kind == PP_LAYOUT_CIRCULAR || kind == PP_LAYOUT_GRID, PP_ERR_ARG, "pp_graph_layout_closed_form: unknown kind %d", kind);
    PP_REQUIRE(n >= 0 && n < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_closed_form: n outside [0, 2^31 - 1)");
    if (n == 0) return PP_OK;
    PP_REQUIRE(pos, PP_ERR_ARG, "pp_graph_layout_closed_form: null pointer");
    k_layout_closed_form<<<capped_grid(n, kBlock), kBlock, 0, (hipStream_t)stream>>>(kind, n, (double2*)pos);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_graph_layout_adj_ws_bytes(int64_t m) { return pp::carve_layout_adj(nullptr, m > 0 ? m : 0).bytes; }

int pp_graph_layout_adj_count(const int64_t* edge_index, int64_t m, int64_t n, int64_t* nnz, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && m >= 0, PP_ERR_ARG, "pp_graph_layout_adj_count: negative size");
    PP_REQUIRE(n < (int64_t)0x7fffffff && 2 * m < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_adj_count: n or 2 m >= 2^31 - 1");
    PP_REQUIRE(nnz, PP_ERR_ARG, "pp_graph_layout_adj_count: nnz is required");
    PP_REQUIRE(ws_bytes >= pp_graph_layout_adj_ws_bytes(m), PP_ERR_WORKSPACE, "pp_graph_layout_adj_count: workspace too small");
    *nnz = 0;
    if (m == 0 || n == 0) return PP_OK;
    PP_REQUIRE(edge_index && ws, PP_ERR_ARG, "pp_graph_layout_adj_count: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const LayoutAdjWs w = carve_layout_adj(ws, m);
    const int64_t count = 2 * m;
    k_layout_adj_keys<<<capped_grid(m, kBlock), kBlock, 0, st>>>(edge_index, m, n, w.key);
    PP_LAUNCH_CHECK();
    int rc = sort_pairs<uint64_t>(w.key, nullptr, w.sorted, w.entry, count, 0, bits_for((uint64_t)n * (uint64_t)n), w.sort, w.sort_bytes, st);
    if (rc != PP_OK) return rc;
    k_layout_adj_flags<<<capped_grid(count, kBlock), kBlock, 0, st>>>(w.sorted, count, n, w.flag);
    PP_LAUNCH_CHECK();
    rc = exclusive_scan<int32_t, int64_t>(w.flag, count, w.pos, true, w.total, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    PP_HIP(hipMemcpyAsync(nnz, w.total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int pp_graph_layout_adj_fill(const double* weight, int64_t m, int64_t n, int64_t nnz, int64_t* ptr, int64_t* nbr, double* w, void* ws,
                             size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && m >= 0 && nnz >= 0 && nnz <= 2 * m, PP_ERR_ARG, "pp_graph_layout_adj_fill: bad sizes");
    PP_REQUIRE(n < (int64_t)0x7fffffff && 2 * m < (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_layout_adj_fill: n or 2 m >= 2^31 - 1");
    PP_REQUIRE(ptr, PP_ERR_ARG, "pp_graph_layout_adj_fill: ptr is required");
    PP_REQUIRE(ws_bytes >= pp_graph_layout_adj_ws_bytes(m), PP_ERR_WORKSPACE, "pp_graph_layout_adj_fill: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (nnz == 0) {
        PP_HIP(hipMemsetAsync(ptr, 0, (size_t)(n + 1) * sizeof(int64_t), st));
        return PP_OK;
    }
    PP_REQUIRE(nbr && w && ws, PP_ERR_ARG, "pp_graph_layout_adj_fill: null pointer");
    const LayoutAdjWs s = carve_layout_adj(ws, m);
    k_layout_adj_fill<<<capped_grid(2 * m, kBlock), kBlock, 0, st>>>(s.sorted, s.entry, s.flag, s.pos, 2 * m, n, m, nnz, weight, s.row, nbr, w);
    PP_LAUNCH_CHECK();
    k_layout_adj_ptr<<<capped_grid(nnz, kBlock), kBlock, 0, st>>>(s.row, nnz, n, ptr);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
