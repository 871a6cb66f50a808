// pathpyg_amd — connected components of a static Graph: labels, sizes, the largest component's nodes and edges.
//
// Reference: connected_components / largest_connected_component, src/pathpyG/algorithms/components.py:14-53 (the edge list goes to the
// host, scipy.sparse.csgraph.connected_components labels it, a Python loop over graph.edges with two dict lookups per edge filters it).
// Here everything is integer work on the device:
//   weak   : lock-free union-find over the stored edge list.  parent[v] <= v at all times (a root is only ever hooked under a SMALLER
//            node), so there are no cycles and a component's root ends up as its smallest node index.  One lane per stored edge: find both
//            roots with path halving, atomicCAS(&parent[hi], hi, lo); a lost CAS means another lane hooked hi, so it is found again from
//            the value the CAS returned.  Before that pass every node is hooked to its smallest smaller neighbour with one atomicMin per
//            edge (behind a plain "is it smaller at all" test): a hub with a large index then has a parent already and its edges hook
//            their OTHER ends, each on a word of its own, instead of all meeting in CAS on the hub's word.
//   strong : forward colouring + backward search (Orzan) with trimming, on the CSR (out-edges) and CSC (in-edges), self-loops ignored.
//            Per round: trim to a fixpoint (an alive node without alive in- or out-neighbour is its own component); colour[v] = v and
//            colour[w] = max(colour[w], colour[v]) along alive edges to a fixpoint (atomicMax; a node pushes only a colour it has not
//            pushed yet); the nodes with colour[v] == v are roots; from all roots at once a search backwards over in-edges inside the
//            root's colour class reaches exactly the root's component, which takes its smallest member as representative (atomicMin on a
//            word per root) and leaves.  Every round removes at least the component of the largest alive node of every colour class.
// Every fixpoint is a HOST loop over launches that reads a device word back; no workgroup waits for another inside a launch.  The loops are
// bounded by n (sweeps <= n + 1 per fixpoint, rounds <= n): past the bound the call fails with PP_ERR_HIP instead of spinning.
// All mutable node state is read with relaxed device-scope atomic loads and written with atomics: a value read late is an OLDER value of a
// monotone word (parent and colour only move one way, marks only rise), which every step tolerates — it is found again, or pushed again in
// the next sweep; a sweep that changed nothing has read exact values, so "no change" is a true fixpoint.  Outputs are therefore independent
// of scheduling.  Rows of 64 entries or more are walked by the whole wave (as expand_frontier in pp_graph_paths.hip does).
#include <limits.h>

#include "pp_common.h"
#include "pp_internal.h"
#include "pp_rows.h"

namespace pp {

__device__ __forceinline__ int32_t ld32(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st32(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------ weak: union-find
__global__ __launch_bounds__(kBlock) void k_cc_identity(int32_t* __restrict__ parent, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) parent[v] = (int32_t)v;
}

__global__ __launch_bounds__(kBlock) void k_cc_hook_smaller(const int64_t* __restrict__ edge_index, int64_t m, int64_t n, int32_t* parent) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t u = edge_index[e], w = edge_index[m + e];
        if ((uint64_t)u >= (uint64_t)n || (uint64_t)w >= (uint64_t)n || u == w) continue;
        const int32_t hi = (int32_t)(u > w ? u : w), lo = (int32_t)(u > w ? w : u);
        if (ld32(parent + hi) > lo) atomicMin(parent + hi, lo);                         // (an older value is a larger one: the test never skips wrongly)
    }
}

// root of x's tree, halving the path on the way (parent[x] = grandparent, by atomicMin: a parent never moves up again)
__device__ __forceinline__ int32_t cc_find(int32_t* parent, int32_t x) {
    int32_t p = ld32(parent + x);
    while (p != x) {                                                                    // x strictly decreases: at most n trips
        const int32_t gp = ld32(parent + p);
        if (gp == p) return p;
        atomicMin(parent + x, gp);
        x = gp;
        p = ld32(parent + x);
    }
    return x;
}

__global__ __launch_bounds__(kBlock) void k_cc_union(const int64_t* __restrict__ edge_index, int64_t m, int64_t n, int32_t* parent) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t u = edge_index[e], w = edge_index[m + e];
        if ((uint64_t)u >= (uint64_t)n || (uint64_t)w >= (uint64_t)n || u == w) continue;
        if (ld32(parent + u) == ld32(parent + w)) continue;                             // same parent: same tree already
        int32_t a = cc_find(parent, (int32_t)u), b = cc_find(parent, (int32_t)w);
        while (a != b) {
            const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
            const int32_t old = atomicCAS(parent + hi, hi, lo);
            if (old == hi) break;                                                       // hooked
            const int32_t again = cc_find(parent, old);                                 // lost: somebody hooked hi under old < hi
            if (hi == a) a = again; else b = again;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_flatten(int32_t* parent, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
        int32_t r = (int32_t)v, p = ld32(parent + r);
        while (p != r) { r = p; p = ld32(parent + r); }
        st32(parent + v, r);                                                            // (the trees are final: a reader meets v's old parent or the root)
    }
}

// ------------------------------------------------------------------ strong: trim, colour, backward search
// visit(node, payload, neighbour) for the entries of the lane's row ptr[v] .. ptr[v + 1] (own lanes only); rows of a wave's width or more are
// walked by the whole wave.  Returns, on the owning lane, whether any visit returned true; kEarly stops a row at the first one.
template <bool kEarly, typename Visit>
__device__ __forceinline__ bool walk_row(const int64_t* __restrict__ ptr, const int64_t* __restrict__ idx, int64_t m, int32_t v, bool own,
                                         int32_t payload, Visit&& visit) {
    int32_t p0 = 0, p1 = 0;
    if (own) {
        int64_t a = ptr[v], b = ptr[v + 1];
        a = a < 0 ? 0 : a;
        b = b > m ? m : b;                                                              // (a row pointer is never trusted past the edge array)
        p0 = (int32_t)a;
        p1 = (int32_t)(b < a ? a : b);
    }
    const bool hub = p1 - p0 >= kWave;
    bool found = false;
    if (!hub)
        for (int32_t p = p0; p < p1; ++p)
            if (visit(v, payload, idx[p])) {
                found = true;
                if (kEarly) break;
            }
    unsigned long long hubs = __ballot(hub);
    while (hubs) {
        const int owner = __ffsll((long long)hubs) - 1;
        hubs &= hubs - 1;
        const int32_t hv = __shfl(v, owner, kWave), h0 = __shfl(p0, owner, kWave), h1 = __shfl(p1, owner, kWave);
        const int32_t hx = __shfl(payload, owner, kWave);
        bool mine = false;
        for (int64_t q = h0; q < h1; q += kWave) {                                      // q is wave-uniform
            const int64_t p = q + lane_id();
            const bool hit = p < h1 && visit(hv, hx, idx[p]);
            mine |= hit;
            if (kEarly && __any(hit)) break;
        }
        const bool any_hit = __any(mine);
        if (lane_id() == owner) found = any_hit;
    }
    return found;
}

// rep[v] < 0: alive.  flags[0]: the number of the last sweep (counted from 1 per fixpoint) that changed something;
// flags[1]: the number of the last trim sweep that left somebody alive.
#define PP_NODE_WAVES(v)                                                                                              \
    for (int64_t base__ = (int64_t)blockIdx.x * kBlock + wave_id() * kWave, v = base__ + lane_id(); base__ < n;      \
         base__ += (int64_t)gridDim.x * kBlock, v = base__ + lane_id())

__global__ __launch_bounds__(kBlock) void k_scc_trim(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                                                    const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ row, int64_t n, int64_t m,
                                                    int32_t* rep, int32_t* flags, int32_t sweep) {
    auto alive_other = [&](int32_t v, int32_t, int64_t w) { return (uint64_t)w < (uint64_t)n && w != v && ld32(rep + w) < 0; };
    bool any = false, stays = false;
    PP_NODE_WAVES(v) {
        const bool alive = v < n && ld32(rep + v) < 0;
        const bool has_in = walk_row<true>(col_ptr, row, m, (int32_t)v, alive, 0, alive_other);
        const bool has_out = walk_row<true>(row_ptr, col, m, (int32_t)v, alive && has_in, 0, alive_other);
        if (alive && !(has_in && has_out)) {
            st32(rep + v, (int32_t)v);
            any = true;
        }
        stays |= alive && has_in && has_out;
    }
    if (any) st32(flags, sweep);
    if (stays) st32(flags + 1, sweep);                                                  // (exact in the sweep that changes nothing: the one the host acts on)
}

__global__ __launch_bounds__(kBlock) void k_scc_colour_init(const int32_t* __restrict__ rep, int64_t n, int32_t* __restrict__ colour,
                                                           int32_t* __restrict__ sent) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
        if (rep[v] < 0) {
            colour[v] = (int32_t)v;
            sent[v] = -1;
        }
}

__global__ __launch_bounds__(kBlock) void k_scc_colour(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col, int64_t n, int64_t m,
                                                      const int32_t* __restrict__ rep, int32_t* colour, int32_t* __restrict__ sent,
                                                      int32_t* flags, int32_t sweep) {
    bool any = false;
    PP_NODE_WAVES(v) {
        int32_t c = -1;
        bool own = v < n && rep[v] < 0;
        if (own) {
            c = ld32(colour + v);
            own = c != sent[v];                                                         // (sent[v] is the owner's alone)
            if (own) { sent[v] = c; any = true; }
        }
        walk_row<false>(row_ptr, col, m, (int32_t)v, own, c, [&](int32_t hv, int32_t hc, int64_t w) {
            if ((uint64_t)w >= (uint64_t)n || w == hv || rep[w] >= 0) return false;
            if (ld32(colour + w) < hc) atomicMax(colour + w, hc);
            return false;
        });
    }
    if (any) st32(flags, sweep);
}

// mark: 0 not reached, 1 reached, 2 reached and expanded.  min_member[r]: smallest member of root r's component.
__global__ __launch_bounds__(kBlock) void k_scc_back_init(const int32_t* __restrict__ rep, const int32_t* __restrict__ colour, int64_t n,
                                                         int32_t* __restrict__ mark, int32_t* __restrict__ min_member) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
        if (rep[v] < 0) {
            mark[v] = colour[v] == (int32_t)v ? 1 : 0;
            min_member[v] = INT_MAX;
        }
}

__global__ __launch_bounds__(kBlock) void k_scc_back(const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ row, int64_t n, int64_t m,
                                                    const int32_t* __restrict__ rep, const int32_t* __restrict__ colour, int32_t* mark,
                                                    int32_t* flags, int32_t sweep) {
    bool any = false;
    PP_NODE_WAVES(v) {
        const bool own = v < n && rep[v] < 0 && ld32(mark + v) == 1;
        int32_t c = -1;
        if (own) {
            c = colour[v];
            st32(mark + v, 2);                                                          // (against an atomicMax(.., 1) of another lane: 2 either way)
            any = true;
        }
        walk_row<false>(col_ptr, row, m, (int32_t)v, own, c, [&](int32_t hv, int32_t hc, int64_t u) {
            if ((uint64_t)u >= (uint64_t)n || u == hv || rep[u] >= 0 || colour[u] != hc) return false;
            if (ld32(mark + u) == 0) atomicMax(mark + u, 1);
            return false;
        });
    }
    if (any) st32(flags, sweep);
}

__global__ __launch_bounds__(kBlock) void k_scc_min_member(const int32_t* __restrict__ rep, const int32_t* __restrict__ colour,
                                                          const int32_t* __restrict__ mark, int64_t n, int32_t* min_member) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
        if (rep[v] < 0 && mark[v] == 2) atomicMin(min_member + colour[v], (int32_t)v);
}

__global__ __launch_bounds__(kBlock) void k_scc_assign(int32_t* __restrict__ rep, const int32_t* __restrict__ colour,
                                                      const int32_t* __restrict__ mark, const int32_t* __restrict__ min_member, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
        if (rep[v] < 0 && mark[v] == 2) rep[v] = min_member[colour[v]];                 // (every lane reads and writes its own rep[v] only)
}

// ------------------------------------------------------------------ shared tail: labels in the order of the smallest member, sizes
__global__ __launch_bounds__(kBlock) void k_cc_is_rep(const int32_t* __restrict__ rep, int64_t n, int32_t* __restrict__ is_rep) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) is_rep[v] = rep[v] == (int32_t)v;
}

__global__ __launch_bounds__(kBlock) void k_cc_labels(const int32_t* __restrict__ rep, const int32_t* __restrict__ rank, int64_t n,
                                                     int32_t* __restrict__ labels, int64_t* sizes) {
    PP_NODE_WAVES(v) {
        int32_t label = -1;
        if (v < n) {
            const int32_t r = rep[v];
            label = (uint32_t)r < (uint32_t)n ? rank[r] : 0;
            labels[v] = label;
        }
        // lanes that share the first active lane's label (a giant component: nearly all of them) add their number once
        const unsigned long long active = __ballot(v < n);
        if (!active) continue;
        const int32_t first = __shfl(label, __ffsll((long long)active) - 1, kWave);
        const unsigned long long same = __ballot(v < n && label == first);
        if (v < n) {
            if (label != first) atomicAdd((unsigned long long*)&sizes[label], 1ull);
            else if (lane_id() == __ffsll((long long)same) - 1) atomicAdd((unsigned long long*)&sizes[label], (unsigned long long)__popcll(same));
        }
    }
}

// out2 = {label, size} of the largest component; among equals the smallest label.  One workgroup.
__global__ __launch_bounds__(kBlock) void k_cc_largest(const int64_t* __restrict__ sizes, const int64_t* __restrict__ count, int64_t* out2) {
    __shared__ int64_t s_size[kBlock], s_label[kBlock];
    const int64_t k = count[0];
    int64_t best = -1, which = -1;
    for (int64_t c = threadIdx.x; c < k; c += kBlock)                                   // ascending labels per thread: '>' keeps the first
        if (sizes[c] > best) { best = sizes[c]; which = c; }
    s_size[threadIdx.x] = best;
    s_label[threadIdx.x] = which;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const int64_t os = s_size[threadIdx.x + d], ol = s_label[threadIdx.x + d];
            if (os > s_size[threadIdx.x] || (os == s_size[threadIdx.x] && ol >= 0 && ol < s_label[threadIdx.x])) {
                s_size[threadIdx.x] = os;
                s_label[threadIdx.x] = ol;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out2[0] = s_label[0]; out2[1] = s_size[0] < 0 ? 0 : s_size[0]; }
}

// ------------------------------------------------------------------ the kept component's nodes and edges, compacted in stored order
__global__ __launch_bounds__(kBlock) void k_cc_keep_nodes(const int32_t* __restrict__ labels, int64_t n, int32_t keep, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) flag[v] = labels[v] == keep;
}

__global__ __launch_bounds__(kBlock) void k_cc_keep_edges(const int64_t* __restrict__ edge_index, int64_t m, int64_t n,
                                                         const int32_t* __restrict__ labels, int32_t keep, int32_t* __restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock) {
        const int64_t u = edge_index[e], w = edge_index[m + e];
        flag[e] = (uint64_t)u < (uint64_t)n && (uint64_t)w < (uint64_t)n && labels[u] == keep && labels[w] == keep;
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_put_nodes(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int64_t n,
                                                        int64_t* __restrict__ nodes_out, int64_t cap) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock)
        if (flag[v] && pos[v] < cap) nodes_out[pos[v]] = v;
}

__global__ __launch_bounds__(kBlock) void k_cc_put_edges(const int64_t* __restrict__ edge_index, int64_t m, const int32_t* __restrict__ flag,
                                                        const int32_t* __restrict__ pos, const int64_t* __restrict__ new_index,
                                                        int64_t* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < m; e += (int64_t)gridDim.x * kBlock)
        if (flag[e]) {                                                                  // (flagged: both ends are in [0, n))
            out[pos[e]] = new_index[edge_index[e]];
            out[m + pos[e]] = new_index[edge_index[m + e]];
        }
}

struct ComponentsWs {
    int32_t *rep, *is_rep, *rank, *flags, *colour, *sent, *mark, *min_member;
    void* scan;
    size_t scan_bytes, total;
};

static ComponentsWs carve_components(void* ws, int64_t n, bool strong) {
    Arena a(ws, 0);
    ComponentsWs w{};
    w.rep = a.take<int32_t>(n);
    w.is_rep = a.take<int32_t>(n);
    w.rank = a.take<int32_t>(n + 1);
    w.flags = a.take<int32_t>(4);
    if (strong) {
        w.colour = a.take<int32_t>(n);
        w.sent = a.take<int32_t>(n);
        w.mark = a.take<int32_t>(n);
        w.min_member = a.take<int32_t>(n);
    }
    w.scan_bytes = scan_ws_bytes(n);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.total = a.used;
    return w;
}

struct KeepWs {
    int32_t *flag, *pos;
    void* scan;
    size_t scan_bytes, total;
};

static KeepWs carve_keep(void* ws, int64_t count) {
    Arena a(ws, 0);
    KeepWs w{};
    w.flag = a.take<int32_t>(count);
    w.pos = a.take<int32_t>(count + 1);
    w.scan_bytes = scan_ws_bytes(count);
    w.scan = a.take<char>((int64_t)w.scan_bytes);
    w.total = a.used;
    return w;
}

// `launch(k)` queues sweep number k = 1, 2, ...; a sweep that changes something stores its number in flags[0].  Sweeps run in growing batches
// between two reads of flags[0..1]: the fixpoint is reached when the LAST sweep of a batch changed nothing.  At most n + 1 sweeps.
template <typename Launch>
static int sweep_to_fixpoint(Launch&& launch, int64_t n, int32_t* flags, int32_t* host_flags, int64_t* sweeps, hipStream_t st, const char* what,
                             int64_t* last_sweep = nullptr) {
    int64_t done = 0, batch = 1;
    PP_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), st));
    for (;;) {
        PP_REQUIRE(done < n + 1, PP_ERR_HIP, "pp_graph_components: %s did not settle within n + 1 = %lld sweeps", what, (long long)(n + 1));
        const int64_t now = batch < n + 1 - done ? batch : n + 1 - done;
        for (int64_t i = 0; i < now; ++i) {
            launch((int32_t)(done + i + 1));
            PP_LAUNCH_CHECK();
        }
        done += now;
        *sweeps += now;
        PP_HIP(hipMemcpyAsync(host_flags, flags, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        if (host_flags[0] != (int32_t)done) {
            if (last_sweep) *last_sweep = done;
            return PP_OK;
        }
        if (batch < 32) batch *= 2;
    }
}

}  // namespace pp

extern "C" {

size_t pp_graph_components_ws_bytes(int64_t n, int64_t m, int strong) {
    (void)m;
    return pp::carve_components(nullptr, n > 0 ? n : 0, strong != 0).total;
}

int pp_graph_components(const int64_t* edge_index, int64_t m, int64_t n, const int64_t* row_ptr, const int64_t* col, const int64_t* col_ptr,
                        const int64_t* row, int strong, int32_t* labels, int64_t* sizes, int64_t* count, int64_t* stats, void* ws,
                        size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(m >= 0 && n >= 0, PP_ERR_ARG, "pp_graph_components: negative size");
    PP_REQUIRE(m <= (int64_t)0x7fffffff && n <= (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_components: size >= 2^31");
    PP_REQUIRE(count != nullptr && (n == 0 || (labels && sizes)), PP_ERR_ARG, "pp_graph_components: labels, sizes and count are required");
    PP_REQUIRE(m == 0 || edge_index, PP_ERR_ARG, "pp_graph_components: edge_index is required");
    PP_REQUIRE(!strong || m == 0 || n == 0 || (row_ptr && col && col_ptr && row), PP_ERR_ARG, "pp_graph_components: strong needs the CSR and the CSC");
    PP_REQUIRE(ws_bytes >= pp_graph_components_ws_bytes(n, m, strong), PP_ERR_WORKSPACE, "pp_graph_components: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int64_t counters[4] = {0, 0, 0, 0};
    if (stats) for (int i = 0; i < 4; ++i) stats[i] = 0;
    if (n == 0) {
        PP_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), st));
        return PP_OK;
    }
    const ComponentsWs w = carve_components(ws, n, strong != 0);
    const unsigned gn = capped_grid(n, kBlock), gm = capped_grid(m, kBlock);
    if (m == 0 || !strong) {
        k_cc_identity<<<gn, kBlock, 0, st>>>(w.rep, n);
        PP_LAUNCH_CHECK();
        if (m > 0) {
            k_cc_hook_smaller<<<gm, kBlock, 0, st>>>(edge_index, m, n, w.rep);
            PP_LAUNCH_CHECK();
            k_cc_union<<<gm, kBlock, 0, st>>>(edge_index, m, n, w.rep);
            PP_LAUNCH_CHECK();
            k_cc_flatten<<<gn, kBlock, 0, st>>>(w.rep, n);
            PP_LAUNCH_CHECK();
        }
    } else {
        int32_t host_flags[2] = {0, 0};
        PP_HIP(hipMemsetAsync(w.rep, 0xff, (size_t)n * sizeof(int32_t), st));           // -1: alive
        for (;;) {
            int64_t last_trim = 0;
            int rc = sweep_to_fixpoint([&](int32_t k) { k_scc_trim<<<gn, kBlock, 0, st>>>(row_ptr, col, col_ptr, row, n, m, w.rep, w.flags, k); }, n, w.flags,
                                       host_flags, &counters[1], st, "trimming", &last_trim);
            if (rc != PP_OK) return rc;
            if (host_flags[1] != (int32_t)last_trim) break;                             // the settled sweep met nobody alive
            PP_REQUIRE(counters[0] < n, PP_ERR_HIP, "pp_graph_components: nodes are still alive after n = %lld rounds", (long long)n);
            ++counters[0];
            k_scc_colour_init<<<gn, kBlock, 0, st>>>(w.rep, n, w.colour, w.sent);
            PP_LAUNCH_CHECK();
            rc = sweep_to_fixpoint([&](int32_t k) { k_scc_colour<<<gn, kBlock, 0, st>>>(row_ptr, col, n, m, w.rep, w.colour, w.sent, w.flags, k); }, n, w.flags,
                                   host_flags, &counters[2], st, "colouring");
            if (rc != PP_OK) return rc;
            k_scc_back_init<<<gn, kBlock, 0, st>>>(w.rep, w.colour, n, w.mark, w.min_member);
            PP_LAUNCH_CHECK();
            rc = sweep_to_fixpoint([&](int32_t k) { k_scc_back<<<gn, kBlock, 0, st>>>(col_ptr, row, n, m, w.rep, w.colour, w.mark, w.flags, k); }, n, w.flags,
                                   host_flags, &counters[3], st, "the backward search");
            if (rc != PP_OK) return rc;
            k_scc_min_member<<<gn, kBlock, 0, st>>>(w.rep, w.colour, w.mark, n, w.min_member);
            PP_LAUNCH_CHECK();
            k_scc_assign<<<gn, kBlock, 0, st>>>(w.rep, w.colour, w.mark, w.min_member, n);
            PP_LAUNCH_CHECK();
        }
        if (stats) for (int i = 0; i < 4; ++i) stats[i] = counters[i];
    }
    k_cc_is_rep<<<gn, kBlock, 0, st>>>(w.rep, n, w.is_rep);
    PP_LAUNCH_CHECK();
    const int rc = exclusive_scan<int32_t, int32_t>(w.is_rep, n, w.rank, true, count, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    PP_HIP(hipMemsetAsync(sizes, 0, (size_t)n * sizeof(int64_t), st));
    k_cc_labels<<<gn, kBlock, 0, st>>>(w.rep, w.rank, n, labels, sizes);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_components_largest(const int64_t* sizes, const int64_t* count, int64_t* out2, pp_stream_t stream) {
    PP_REQUIRE(sizes && count && out2, PP_ERR_ARG, "pp_graph_components_largest: null argument");
    pp::k_cc_largest<<<1, pp::kBlock, 0, (hipStream_t)stream>>>(sizes, count, out2);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

size_t pp_graph_component_keep_ws_bytes(int64_t count) { return pp::carve_keep(nullptr, count > 0 ? count : 0).total; }

int pp_graph_component_nodes(const int32_t* labels, int64_t n, int64_t keep, int64_t* nodes_out, int64_t nodes_cap, int64_t* count_out, void* ws,
                             size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(n >= 0 && nodes_cap >= 0, PP_ERR_ARG, "pp_graph_component_nodes: negative size");
    PP_REQUIRE(n <= (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_component_nodes: size >= 2^31");
    PP_REQUIRE(count_out != nullptr, PP_ERR_ARG, "pp_graph_component_nodes: count_out is required");
    PP_REQUIRE(ws_bytes >= pp_graph_component_keep_ws_bytes(n), PP_ERR_WORKSPACE, "pp_graph_component_nodes: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || keep < 0 || keep > (int64_t)0x7fffffff) {
        PP_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), st));
        return PP_OK;
    }
    const KeepWs w = carve_keep(ws, n);
    k_cc_keep_nodes<<<capped_grid(n, kBlock), kBlock, 0, st>>>(labels, n, (int32_t)keep, w.flag);
    PP_LAUNCH_CHECK();
    const int rc = exclusive_scan<int32_t, int32_t>(w.flag, n, w.pos, true, count_out, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    k_cc_put_nodes<<<capped_grid(n, kBlock), kBlock, 0, st>>>(w.flag, w.pos, n, nodes_out, nodes_cap);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_graph_component_edges(const int64_t* edge_index, int64_t m, int64_t n, const int32_t* labels, int64_t keep, const int64_t* new_index,
                             int64_t* edges_out, int64_t* count_out, void* ws, size_t ws_bytes, pp_stream_t stream) {
    using namespace pp;
    PP_REQUIRE(m >= 0 && n >= 0, PP_ERR_ARG, "pp_graph_component_edges: negative size");
    PP_REQUIRE(m <= (int64_t)0x7fffffff && n <= (int64_t)0x7fffffff, PP_ERR_TOO_LARGE, "pp_graph_component_edges: size >= 2^31");
    PP_REQUIRE(count_out != nullptr, PP_ERR_ARG, "pp_graph_component_edges: count_out is required");
    PP_REQUIRE(ws_bytes >= pp_graph_component_keep_ws_bytes(m), PP_ERR_WORKSPACE, "pp_graph_component_edges: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    if (m == 0 || n == 0 || keep < 0 || keep > (int64_t)0x7fffffff) {
        PP_HIP(hipMemsetAsync(count_out, 0, sizeof(int64_t), st));
        return PP_OK;
    }
    const KeepWs w = carve_keep(ws, m);
    k_cc_keep_edges<<<capped_grid(m, kBlock), kBlock, 0, st>>>(edge_index, m, n, labels, (int32_t)keep, w.flag);
    PP_LAUNCH_CHECK();
    const int rc = exclusive_scan<int32_t, int32_t>(w.flag, m, w.pos, true, count_out, w.scan, w.scan_bytes, st);
    if (rc != PP_OK) return rc;
    k_cc_put_edges<<<capped_grid(m, kBlock), kBlock, 0, st>>>(edge_index, m, w.flag, w.pos, new_index, edges_out);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
