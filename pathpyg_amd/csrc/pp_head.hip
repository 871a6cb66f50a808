// pathpyg_amd — the head of the DBGNN on the first-order rows, one kernel forward and one backward.
//
// Reference code replaced (paths relative to the pathpyG repository root):
//   BipartiteGraphOperator.forward / message    src/pathpyG/nn/dbgnn.py:66-69     (after the re-association of lin1: the sum over the
//   DBGNN.forward, bipartite ELU + classifier   src/pathpyG/nn/dbgnn.py:143-151    higher-order rows `agg` is formed first, pp_spmm_f32)
//
//     z      = ELU( agg . W1^T + deg (*) (x . W2^T + b2 + b1) )          agg [n,HA], x [n,HX] (a stored ELU activation), deg [n]
//     logits = z . Wlin^T + blin                                          z [n,HB], logits [n,C], C <= 16
//
// As a chain of kernels (pp_dense_f32 twice, pp_bip_combine_f32, pp_dense_narrow_f32 and their backward kernels) every intermediate is
// an n x 64 matrix written by one kernel and read by the next; here a wave owns a 16-row tile from its inputs to its outputs and the
// intermediates live in registers.  v_mfma_f32_16x16x4_f32 throughout: A operand = lane (i = lane&15, kq = lane>>4) holds A[i][kq],
// B operand = B[kq][i], C/D = row 4*kq + reg, column i.  Two freedoms of that layout keep every global access a 16-byte one:
//   * the k order of a dot product is free: k-step (c, e) takes k = 16c + 4kq + e, so a lane's A values are float4 pieces of its row
//     and the four kq lanes of a row read 64 contiguous bytes;
//   * the column a lane owns in output tile ct is free: it is CT*i + ct (CT = width / 16), so the CT tiles of a lane are CT consecutive
//     floats of a row.  The weights are loaded into the B registers in the matching order once per (persistent) wave.
#include "pp_internal.h"

namespace pp {

using head_f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kHeadMaxBlocks = 512;                  // partial weight-gradient tiles per matrix (2 workgroups per CU)
constexpr int kHeadSlices = 16;                      // k_head_reduce: partial tiles are summed in 16 interleaved slices, then slice by slice

// CT consecutive floats of a row (a lane's columns CT*i .. CT*i + CT - 1); rows past the end read as zeros
template <int CT>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, bool live, float (&v)[CT]) {
    if constexpr (CT == 4) {
        const float4 t = live ? *(const float4*)p : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if constexpr (CT == 2) {
        const float2 t = live ? *(const float2*)p : make_float2(0.f, 0.f);
        v[0] = t.x; v[1] = t.y;
    } else {
        v[0] = live ? p[0] : 0.f;
    }
}

template <int CT>
__device__ __forceinline__ void store_cols(float* __restrict__ p, const float (&v)[CT]) {
    if constexpr (CT == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    else if constexpr (CT == 2) *(float2*)p = make_float2(v[0], v[1]);
    else p[0] = v[0];
}

__device__ __forceinline__ float elu_grad(float y) { return y > 0.f ? 1.f : y + 1.f; }      // ELU'(pre) from the stored y = ELU(pre)

// ------------------------------------------------------------------ forward
template <int HA, int HX, int HB>
__global__ __launch_bounds__(kBlock, 2) void k_head_forward(const float* __restrict__ agg, const float* __restrict__ x, const float* __restrict__ deg,
                                                        const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                                        const float* __restrict__ b2, const float* __restrict__ Wlin, const float* __restrict__ blin,
                                                        int64_t n_rows, int C, float* __restrict__ z, float* __restrict__ logits) {
    constexpr int FA = HA / 16, FX = HX / 16, FB = HB / 16;         // float4 pieces per lane and row; FB = output tiles
    constexpr int TS = HB + 4;                                      // row stride of the LDS tile
    __shared__ __attribute__((aligned(16))) float s_z[kWavesPerBlock][16 * TS];    // wave-private: z tile, C layout -> A layout
    const int lane = lane_id(), i = lane & 15, kq = lane >> 4;
    float* tile_z = s_z[wave_id()];
    // Wlin^T as B operand (row i = class i, zero beyond C) stays in LDS: 16 registers less keep the kernel at 2 waves per SIMD without spills
    __shared__ __attribute__((aligned(16))) float s_wl[16 * TS];
    for (int e = threadIdx.x; e < 16 * HB; e += kBlock) s_wl[(e / HB) * TS + e % HB] = e / HB < C ? Wlin[e] : 0.f;
    __syncthreads();
    float w1[FA * 4][FB], w2[FX * 4][FB], bsum[FB];
#pragma unroll
    for (int ct = 0; ct < FB; ++ct) {
        const int j = FB * i + ct;
#pragma unroll
        for (int t = 0; t < FA * 4; ++t) w1[t][ct] = W1[j * HA + 16 * (t / 4) + 4 * kq + t % 4];
#pragma unroll
        for (int t = 0; t < FX * 4; ++t) w2[t][ct] = W2[j * HX + 16 * (t / 4) + 4 * kq + t % 4];
        bsum[ct] = b1[j] + b2[j];
    }
    const float bl = i < C ? blin[i] : 0.f;

    const int64_t n_tiles = (n_rows + 15) / 16;
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + wave_id();
    float4 a_cur[FA], a_nxt[FA], x_cur[FX], x_nxt[FX];
    float d_cur, d_nxt;
    auto load_tile = [&](int64_t t, float4 (&a)[FA], float4 (&xv)[FX], float& d) {
        const int64_t r = t * 16 + i;
        const bool live = t < n_tiles && r < n_rows;
#pragma unroll
        for (int c = 0; c < FA; ++c) a[c] = live ? *(const float4*)(agg + r * HA + 16 * c + 4 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < FX; ++c) xv[c] = live ? *(const float4*)(x + r * HX + 16 * c + 4 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        d = live ? deg[r] : 0.f;
    };
    load_tile(tile, a_cur, x_cur, d_cur);
    for (; tile < n_tiles; tile += n_waves) {
        load_tile(tile + n_waves, a_nxt, x_nxt, d_nxt);
        // agg . W1^T + (deg (*) x) . W2^T in ONE accumulator set
        head_f32x4 acc[FB];
#pragma unroll
        for (int ct = 0; ct < FB; ++ct) acc[ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < FA; ++c) {
            const float av[4] = {a_cur[c].x, a_cur[c].y, a_cur[c].z, a_cur[c].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ct = 0; ct < FB; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], w1[4 * c + e][ct], acc[ct], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < FX; ++c) {
            const float xv[4] = {d_cur * x_cur[c].x, d_cur * x_cur[c].y, d_cur * x_cur[c].z, d_cur * x_cur[c].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ct = 0; ct < FB; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[e], w2[4 * c + e][ct], acc[ct], 0, 0, 0);
        }
        // combine + ELU in registers (C layout: rows 4*kq + reg, columns FB*i ..); z goes to memory once and to the wave's LDS tile
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float dr = __shfl(d_cur, 4 * kq + reg, kWave);              // lanes 0..15 hold deg of the tile's rows 0..15
            const int64_t r = tile * 16 + 4 * kq + reg;
            float zv[FB];
#pragma unroll
            for (int ct = 0; ct < FB; ++ct) zv[ct] = elu_fast(acc[ct][reg] + dr * bsum[ct]);
            store_cols<FB>(tile_z + (4 * kq + reg) * TS + FB * i, zv);
            if (r < n_rows) store_cols<FB>(z + r * HB + FB * i, zv);
        }
        __builtin_amdgcn_wave_barrier();
        // logits = z . Wlin^T: the z tile in A layout (row i, k = 16c + 4kq + e), two accumulators against the dependent-MFMA latency
        head_f32x4 lg0 = head_f32x4{0.f, 0.f, 0.f, 0.f}, lg1 = head_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < FB; ++c) {
            const float4 t = *(const float4*)(tile_z + i * TS + 16 * c + 4 * kq);
            const float4 wl = *(const float4*)(s_wl + i * TS + 16 * c + 4 * kq);
            lg0 = __builtin_amdgcn_mfma_f32_16x16x4f32(t.x, wl.x, lg0, 0, 0, 0);
            lg1 = __builtin_amdgcn_mfma_f32_16x16x4f32(t.y, wl.y, lg1, 0, 0, 0);
            lg0 = __builtin_amdgcn_mfma_f32_16x16x4f32(t.z, wl.z, lg0, 0, 0, 0);
            lg1 = __builtin_amdgcn_mfma_f32_16x16x4f32(t.w, wl.w, lg1, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
        if (i < C) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t r = tile * 16 + 4 * kq + reg;
                if (r < n_rows) logits[r * C + i] = lg0[reg] + lg1[reg] + bl;
            }
        }
#pragma unroll
        for (int c = 0; c < FA; ++c) a_cur[c] = a_nxt[c];
#pragma unroll
        for (int c = 0; c < FX; ++c) x_cur[c] = x_nxt[c];
        d_cur = d_nxt;
    }
}

// ------------------------------------------------------------------ backward
// The 4 waves' weight-gradient accumulators (C layout: row MT*(4kq + reg) + mt, column CT*i + ct) and column sums are added into one
// zero-padded [64][64] tile (+ [64] sums) per workgroup in wave order; k_head_reduce sums the workgroups' tiles in a fixed order.
template <int MT, int CT, int NB>
__device__ __forceinline__ void head_fold(const head_f32x4 (&acc)[MT][CT], const float (&col)[NB], bool with_col, float* s_tile, float* s_bias,
                                          float* __restrict__ out_w, float* __restrict__ out_b) {
    const int lane = lane_id(), i = lane & 15, kq = lane >> 4;
    for (int e = threadIdx.x; e < 64 * 64; e += kBlock) s_tile[e] = 0.f;
    if (threadIdx.x < 64) s_bias[threadIdx.x] = 0.f;
    __syncthreads();
    for (int w = 0; w < kWavesPerBlock; ++w) {
        if (wave_id() == w) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) s_tile[(MT * (4 * kq + reg) + mt) * 64 + CT * i + ct] += acc[mt][ct][reg];
            if (with_col) {
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    float v = col[q];
                    v += __shfl_xor(v, 16, kWave);
                    v += __shfl_xor(v, 32, kWave);
                    if (kq == 0) s_bias[NB * i + q] += v;
                }
            }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < MT * 16 * 64; e += kBlock) out_w[e] = s_tile[e];
    if (with_col && threadIdx.x < 64) out_b[threadIdx.x] = s_bias[threadIdx.x];
    __syncthreads();
}

struct HeadPartials {
    float *w1, *w2, *wl;         // [blocks][64 * 64] each
    float *b, *bl;               // [blocks][64]: column sums of dper (db1 = db2) and of dlogits (dblin)
};

// One wave per SIMD: the two 64 x 64 weight-gradient accumulator sets and the two weight matrices are 256 registers of the 450 a lane
// holds.  (Split into an `agg` side and an `x` side of 2 waves per SIMD each, every side forming dpre itself, the pair took 420 us
// against 302 us at 5 * 10^5 rows: DESIGN 5.)
template <int HA, int HX, int HB>
__global__ __launch_bounds__(kBlock) void k_head_backward(const float* __restrict__ dlogits, const float* __restrict__ z, const float* __restrict__ agg,
                                                         const float* __restrict__ x, const float* __restrict__ deg, const float* __restrict__ W1,
                                                         const float* __restrict__ W2, const float* __restrict__ Wlin, int64_t n_rows, int C,
                                                         float* __restrict__ d_agg, float* __restrict__ dpre_fo, float* __restrict__ colsum_fo,
                                                         HeadPartials part) {
    constexpr int FA = HA / 16, FX = HX / 16, FB = HB / 16;
    constexpr int TS = HB + 4;
    __shared__ __attribute__((aligned(16))) float s_g[kWavesPerBlock][16 * TS];     // wave-private: dpre tile, C layout -> A layout
    __shared__ float s_tile[64 * 64];
    __shared__ float s_bias[64];
    const int lane = lane_id(), i = lane & 15, kq = lane >> 4;
    float* tile_g = s_g[wave_id()];
    // B operands: Wlin [C,HB] (k = class 4kq + t), W1 [HB,HA] and W2 [HB,HX] (k = 16c + 4kq + e), columns in the lane's CT*i + ct order
    float bl[4][FB], w1[FB * 4][FA], w2[FB * 4][FX];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ct = 0; ct < FB; ++ct) bl[t][ct] = 4 * kq + t < C ? Wlin[(4 * kq + t) * HB + FB * i + ct] : 0.f;
#pragma unroll
    for (int t = 0; t < FB * 4; ++t) {
        const int k = 16 * (t / 4) + 4 * kq + t % 4;
#pragma unroll
        for (int ct = 0; ct < FA; ++ct) w1[t][ct] = W1[k * HA + FA * i + ct];
#pragma unroll
        for (int ct = 0; ct < FX; ++ct) w2[t][ct] = W2[k * HX + FX * i + ct];
    }
    head_f32x4 acc_w1[FB][FA], acc_w2[FB][FX], acc_wl[1][FB];
#pragma unroll
    for (int mt = 0; mt < FB; ++mt) {
#pragma unroll
        for (int ct = 0; ct < FA; ++ct) acc_w1[mt][ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ct = 0; ct < FX; ++ct) acc_w2[mt][ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ct = 0; ct < FB; ++ct) acc_wl[0][ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
    float col_fo[FX], col_b[FB], col_l[1] = {0.f};
#pragma unroll
    for (int ct = 0; ct < FX; ++ct) col_fo[ct] = 0.f;
#pragma unroll
    for (int ct = 0; ct < FB; ++ct) col_b[ct] = 0.f;

    const int64_t n_tiles = (n_rows + 15) / 16;
    const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + wave_id(); tile < n_tiles; tile += n_waves) {
        // ---- this tile's rows: dlogits in A layout (row i, classes 4kq ..), everything else in C layout (rows 4kq + reg, a lane's columns)
        const int64_t ri = tile * 16 + i;
        float dl_a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) dl_a[t] = (ri < n_rows && 4 * kq + t < C) ? dlogits[ri * C + 4 * kq + t] : 0.f;
        const float deg_i = ri < n_rows ? deg[ri] : 0.f;
        float zr[4][FB];
        float ar[4][FA], xr[4][FX], dl_n[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = tile * 16 + 4 * kq + reg;
            const bool live = r < n_rows;
            load_cols<FB>(z + r * HB + FB * i, live, zr[reg]);
            load_cols<FA>(agg + r * HA + FA * i, live, ar[reg]);
            load_cols<FX>(x + r * HX + FX * i, live, xr[reg]);
            dl_n[reg] = (live && i < C) ? dlogits[r * C + i] : 0.f;
        }
        // ---- dz = dlogits . Wlin, dpre = dz (*) ELU'(z)
        head_f32x4 dz[FB];
#pragma unroll
        for (int ct = 0; ct < FB; ++ct) dz[ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ct = 0; ct < FB; ++ct) dz[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(dl_a[t], bl[t][ct], dz[ct], 0, 0, 0);
        float g[4][FB];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
            for (int ct = 0; ct < FB; ++ct) g[reg][ct] = dz[ct][reg] * elu_grad(zr[reg][ct]);
            store_cols<FB>(tile_g + (4 * kq + reg) * TS + FB * i, g[reg]);
        }
        __builtin_amdgcn_wave_barrier();
        float4 g_a[FB];                                           // dpre in A layout: row i, k = 16c + 4kq + e
#pragma unroll
        for (int c = 0; c < FB; ++c) g_a[c] = *(const float4*)(tile_g + i * TS + 16 * c + 4 * kq);
        __builtin_amdgcn_wave_barrier();
        {
            // ---- d_agg = dpre . W1;  dW1 += dpre^T agg (the contraction runs over the tile's rows: step `reg` takes rows {reg, 4+reg, 8+reg, 12+reg});
            //      dWlin += dlogits^T z
            head_f32x4 da[FA];
#pragma unroll
            for (int ct = 0; ct < FA; ++ct) da[ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < FB; ++c) {
                const float gv[4] = {g_a[c].x, g_a[c].y, g_a[c].z, g_a[c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ct = 0; ct < FA; ++ct) da[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[e], w1[4 * c + e][ct], da[ct], 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
                for (int mt = 0; mt < FB; ++mt)
#pragma unroll
                    for (int ct = 0; ct < FA; ++ct)
                        acc_w1[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[reg][mt], ar[reg][ct], acc_w1[mt][ct], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < FB; ++ct) acc_wl[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(dl_n[reg], zr[reg][ct], acc_wl[0][ct], 0, 0, 0);
                col_l[0] += dl_n[reg];
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t r = tile * 16 + 4 * kq + reg;
                float v[FA];
#pragma unroll
                for (int ct = 0; ct < FA; ++ct) v[ct] = da[ct][reg];
                if (r < n_rows) store_cols<FA>(d_agg + r * HA + FA * i, v);
            }
        }
        {
            // ---- dper = deg (*) dpre;  dpre_fo = (dper . W2) (*) ELU'(x);  dW2 += dper^T x;  column sums of dper and dpre_fo
            head_f32x4 dx[FX];
#pragma unroll
            for (int ct = 0; ct < FX; ++ct) dx[ct] = head_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < FB; ++c) {
                const float gv[4] = {deg_i * g_a[c].x, deg_i * g_a[c].y, deg_i * g_a[c].z, deg_i * g_a[c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ct = 0; ct < FX; ++ct) dx[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[e], w2[4 * c + e][ct], dx[ct], 0, 0, 0);
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float dr = __shfl(deg_i, 4 * kq + reg, kWave);          // lanes 0..15 hold deg of the tile's rows 0..15
#pragma unroll
                for (int mt = 0; mt < FB; ++mt) {
                    const float gp = dr * g[reg][mt];
                    col_b[mt] += gp;
#pragma unroll
                    for (int ct = 0; ct < FX; ++ct) acc_w2[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(gp, xr[reg][ct], acc_w2[mt][ct], 0, 0, 0);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t r = tile * 16 + 4 * kq + reg;
                float v[FX];
#pragma unroll
                for (int ct = 0; ct < FX; ++ct) {
                    v[ct] = dx[ct][reg] * elu_grad(xr[reg][ct]);            // (rows past the end: dlogits read as 0, so v == 0)
                    col_fo[ct] += v[ct];
                }
                if (r < n_rows) store_cols<FX>(dpre_fo + r * HX + FX * i, v);
            }
        }
    }
    if (colsum_fo) {
#pragma unroll
        for (int ct = 0; ct < FX; ++ct) {
            float v = col_fo[ct];
            v += __shfl_xor(v, 16, kWave);
            v += __shfl_xor(v, 32, kWave);
            if (kq == 0) atomicAdd(&colsum_fo[FX * i + ct], v);
        }
    }
    const int64_t b = blockIdx.x;
    head_fold<FB, FA, FB>(acc_w1, col_b, false, s_tile, s_bias, part.w1 + (b << 12), nullptr);
    head_fold<FB, FX, FB>(acc_w2, col_b, true, s_tile, s_bias, part.w2 + (b << 12), part.b + b * 64);
    head_fold<1, FB, 1>(acc_wl, col_l, true, s_tile, s_bias, part.wl + (b << 12), part.bl + b * 64);
}

// dW[i][j] = sum over the workgroups' partial tiles (slice g takes tiles g, g + 16, ..; the 16 slice sums are then added in slice order:
// the order k_weight_grad_reduce uses), db likewise from the [64] column sums.  blockIdx.y = matrix.
struct HeadReduceJob {
    const float *partial, *partial_b;
    float *dW, *db, *db_copy;
    int M, K, n_parts;
};
struct HeadReduceJobs {
    HeadReduceJob job[3];
};
__global__ __launch_bounds__(kBlock) void k_head_reduce(HeadReduceJobs jobs) {
    __shared__ float s_sum[kHeadSlices][kBlock / kHeadSlices];
    const HeadReduceJob J = jobs.job[blockIdx.y];
    const int o = threadIdx.x % (kBlock / kHeadSlices), g = threadIdx.x / (kBlock / kHeadSlices);
    const int idx = blockIdx.x * (kBlock / kHeadSlices) + o;          // output element (weights first, then the column sums)
    const int n_w = J.M * J.K;
    float s = 0.f;
    if (idx < n_w) {
        const float* p = J.partial + (idx / J.K) * 64 + idx % J.K;
        for (int64_t w = g; w < J.n_parts; w += kHeadSlices) s += p[w << 12];
    } else if (J.db && idx < n_w + J.M) {
        const float* p = J.partial_b + (idx - n_w);
        for (int64_t w = g; w < J.n_parts; w += kHeadSlices) s += p[w * 64];
    }
    s_sum[g][o] = s;
    __syncthreads();
    if (g == 0) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < kHeadSlices; ++q) t += s_sum[q][o];
        if (idx < n_w) J.dW[idx] = t;
        else if (J.db && idx < n_w + J.M) {
            J.db[idx - n_w] = t;
            if (J.db_copy) J.db_copy[idx - n_w] = t;
        }
    }
}

// persistent grid: what is resident at once (asked from the runtime once per kernel), never more than the partial tiles provide
template <typename Kernel>
static int head_resident(Kernel kernel, int* cache) {
    if (*cache == 0) {
        int per_cu = 0, dev = 0, cus = 0;
        PP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0));
        PP_HIP(hipGetDevice(&dev));
        PP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        *cache = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 256);
    }
    return PP_OK;
}

static inline int64_t head_blocks(int64_t n_rows, int resident, int64_t cap) {
    int64_t blocks = ceil_div(ceil_div(n_rows > 0 ? n_rows : 1, 16), kWavesPerBlock);
    const int64_t share = shared_grid(resident);
    if (blocks > share) blocks = share;
    if (blocks > cap) blocks = cap;
    note_persistent_grid(blocks);
    return blocks;
}

template <int HA, int HX, int HB>
static int launch_head_forward(hipStream_t st, const float* agg, const float* x, const float* deg, const float* W1, const float* b1, const float* W2,
                               const float* b2, const float* Wlin, const float* blin, int64_t n_rows, int C, float* z, float* logits) {
    static int resident = 0;
    const int rc = head_resident(k_head_forward<HA, HX, HB>, &resident);
    if (rc != PP_OK) return rc;
    const int64_t blocks = head_blocks(n_rows, resident, (int64_t)1 << 20);
    k_head_forward<HA, HX, HB><<<(unsigned)blocks, kBlock, 0, st>>>(agg, x, deg, W1, b1, W2, b2, Wlin, blin, n_rows, C, z, logits);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

template <int HA, int HX, int HB>
static int launch_head_backward(hipStream_t st, const float* dlogits, const float* z, const float* agg, const float* x, const float* deg,
                                const float* W1, const float* W2, const float* Wlin, int64_t n_rows, int C, float* d_agg, float* dpre_fo,
                                float* colsum_fo, HeadPartials part, int64_t* blocks_out) {
    static int resident = 0;
    const int rc = head_resident(k_head_backward<HA, HX, HB>, &resident);
    if (rc != PP_OK) return rc;
    const int64_t blocks = head_blocks(n_rows, resident, kHeadMaxBlocks);
    k_head_backward<HA, HX, HB><<<(unsigned)blocks, kBlock, 0, st>>>(dlogits, z, agg, x, deg, W1, W2, Wlin, n_rows, C, d_agg, dpre_fo, colsum_fo,
                                                                          part);
    PP_LAUNCH_CHECK();
    *blocks_out = blocks;
    return PP_OK;
}

static inline bool head_width(int h) { return h == 16 || h == 32 || h == 64; }

}  // namespace pp

using namespace pp;

extern "C" {

int pp_dbgnn_head_supported(int Ha, int Hx, int Hb, int C) { return head_width(Ha) && head_width(Hx) && head_width(Hb) && C >= 1 && C <= 16; }

// every combination of the three widths: PP_HEAD_SHAPES(F) expands F(HA, HX, HB) 27 times
#define PP_HEAD_B(F, A, X) F(A, X, 16) F(A, X, 32) F(A, X, 64)
#define PP_HEAD_X(F, A) PP_HEAD_B(F, A, 16) PP_HEAD_B(F, A, 32) PP_HEAD_B(F, A, 64)
#define PP_HEAD_SHAPES(F) PP_HEAD_X(F, 16) PP_HEAD_X(F, 32) PP_HEAD_X(F, 64)

int pp_dbgnn_head_forward_f32(const float* agg, const float* x, const float* deg, const float* W1, const float* b1, const float* W2, const float* b2,
                              const float* Wlin, const float* blin, int64_t n_rows, int Ha, int Hx, int Hb, int C, float* z, float* logits,
                              pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_rows >= 0, PP_ERR_ARG, "pp_dbgnn_head_forward_f32: negative size");
    PP_REQUIRE(pp_dbgnn_head_supported(Ha, Hx, Hb, C), PP_ERR_ARG,
               "pp_dbgnn_head_forward_f32: unsupported shape %d/%d -> %d -> %d (widths 16/32/64, at most 16 classes)", Ha, Hx, Hb, C);
    if (n_rows == 0) return PP_OK;
    PP_REQUIRE(agg && x && deg && W1 && b1 && W2 && b2 && Wlin && blin && z && logits, PP_ERR_ARG, "pp_dbgnn_head_forward_f32: null argument");
    PP_REQUIRE(((uintptr_t)agg | (uintptr_t)x | (uintptr_t)z) % 16 == 0, PP_ERR_ARG, "pp_dbgnn_head_forward_f32: agg, x and z must be 16-byte aligned");
#define PP_HEAD_FWD(A, X, B) \
    if (Ha == A && Hx == X && Hb == B) return launch_head_forward<A, X, B>(st, agg, x, deg, W1, b1, W2, b2, Wlin, blin, n_rows, C, z, logits);
    PP_HEAD_SHAPES(PP_HEAD_FWD)
#undef PP_HEAD_FWD
    return PP_ERR_ARG;
}

size_t pp_dbgnn_head_backward_ws_bytes(int64_t n_rows) {
    int64_t blocks = ceil_div(ceil_div(n_rows > 0 ? n_rows : 1, 16), kWavesPerBlock);
    if (blocks > kHeadMaxBlocks) blocks = kHeadMaxBlocks;
    return 3 * align_up((size_t)blocks * 4096 * sizeof(float)) + 2 * align_up((size_t)blocks * 64 * sizeof(float));
}

int pp_dbgnn_head_backward_f32(const float* dlogits, const float* z, const float* agg, const float* x, const float* deg, const float* W1,
                               const float* W2, const float* Wlin, int64_t n_rows, int Ha, int Hx, int Hb, int C, float* d_agg,
                               float* dpre_fo, float* colsum_fo, float* dW1, float* dW2, float* db1, float* db2, float* dWlin, float* dblin,
                               void* ws, size_t ws_bytes, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n_rows >= 0, PP_ERR_ARG, "pp_dbgnn_head_backward_f32: negative size");
    PP_REQUIRE(pp_dbgnn_head_supported(Ha, Hx, Hb, C), PP_ERR_ARG,
               "pp_dbgnn_head_backward_f32: unsupported shape %d/%d -> %d -> %d (widths 16/32/64, at most 16 classes)", Ha, Hx, Hb, C);
    PP_REQUIRE(W1 && W2 && Wlin && dW1 && dW2 && db1 && dWlin && dblin, PP_ERR_ARG, "pp_dbgnn_head_backward_f32: null argument");
    if (n_rows == 0) {                                   // no rows: every sum is empty
        PP_HIP(hipMemsetAsync(dW1, 0, (size_t)Hb * Ha * sizeof(float), st));
        PP_HIP(hipMemsetAsync(dW2, 0, (size_t)Hb * Hx * sizeof(float), st));
        PP_HIP(hipMemsetAsync(dWlin, 0, (size_t)C * Hb * sizeof(float), st));
        PP_HIP(hipMemsetAsync(db1, 0, (size_t)Hb * sizeof(float), st));
        if (db2) PP_HIP(hipMemsetAsync(db2, 0, (size_t)Hb * sizeof(float), st));
        PP_HIP(hipMemsetAsync(dblin, 0, (size_t)C * sizeof(float), st));
        if (colsum_fo) PP_HIP(hipMemsetAsync(colsum_fo, 0, (size_t)Hx * sizeof(float), st));
        return PP_OK;
    }
    PP_REQUIRE(dlogits && z && agg && x && deg && d_agg && dpre_fo, PP_ERR_ARG, "pp_dbgnn_head_backward_f32: null argument");
    PP_REQUIRE(((uintptr_t)z | (uintptr_t)agg | (uintptr_t)x | (uintptr_t)d_agg | (uintptr_t)dpre_fo) % 16 == 0, PP_ERR_ARG,
               "pp_dbgnn_head_backward_f32: z, agg, x, d_agg and dpre_fo must be 16-byte aligned");
    PP_REQUIRE(ws != nullptr && ws_bytes >= pp_dbgnn_head_backward_ws_bytes(n_rows), PP_ERR_WORKSPACE, "pp_dbgnn_head_backward_f32: workspace too small");
    if (colsum_fo) PP_HIP(hipMemsetAsync(colsum_fo, 0, (size_t)Hx * sizeof(float), st));
    int64_t cap = ceil_div(ceil_div(n_rows > 0 ? n_rows : 1, 16), kWavesPerBlock);
    if (cap > kHeadMaxBlocks) cap = kHeadMaxBlocks;
    Arena a(ws, ws_bytes);
    HeadPartials part;
    part.w1 = a.take<float>(cap * 4096);
    part.w2 = a.take<float>(cap * 4096);
    part.wl = a.take<float>(cap * 4096);
    part.b = a.take<float>(cap * 64);
    part.bl = a.take<float>(cap * 64);
    int64_t blocks = 0;
    int rc = PP_ERR_ARG;
#define PP_HEAD_BWD(A, X, B) \
    if (Ha == A && Hx == X && Hb == B) \
        rc = launch_head_backward<A, X, B>(st, dlogits, z, agg, x, deg, W1, W2, Wlin, n_rows, C, d_agg, dpre_fo, colsum_fo, part, &blocks);
    PP_HEAD_SHAPES(PP_HEAD_BWD)
#undef PP_HEAD_BWD
    if (rc != PP_OK) return rc;
    HeadReduceJobs jobs;
    jobs.job[0] = HeadReduceJob{part.w1, nullptr, dW1, nullptr, nullptr, Hb, Ha, (int)blocks};
    jobs.job[1] = HeadReduceJob{part.w2, part.b, dW2, db1, db2, Hb, Hx, (int)blocks};
    jobs.job[2] = HeadReduceJob{part.wl, part.bl, dWlin, dblin, nullptr, C, Hb, (int)blocks};
    const int outs = Hb * (Ha > Hx ? Ha : Hx) + Hb;
    k_head_reduce<<<dim3((unsigned)ceil_div(outs, kBlock / kHeadSlices), 3), kBlock, 0, st>>>(jobs);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // extern "C"
