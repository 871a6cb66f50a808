// pathpyg_amd — the loss and the scores of a SEMI-SUPERVISED node classifier (gfx950): softmax cross-entropy over the rows a boolean mask
// and / or an ignore_index select, with class weights, and the confusion matrix of the predictions under the same selection.
//
// The DBGNN is trained on out[train_mask] against y[train_mask] and scored on test_mask (the reference's tutorial loop,
// docs/tutorial/netzschleuder.ipynb cells 15-17).  Written with torch that is a boolean-index gather (with the nonzero read-back that sizes
// it), the generic nll_loss and an index_put backward into a zeroed [N, C]; here the selection is a predicate inside ONE pass over the
// rows, which writes the whole [N, C] gradient (exact zeros on unselected rows) and needs no read-back.
//
// Selection:  row i counts iff (mask == NULL or mask[i] != 0) and (ignore_index unused or target[i] != ignore_index).
// A selected row whose target lies outside [0, C) contributes nothing, gets a zero gradient row and is counted; neither target[i] nor
// weight[target[i]] is used as an index before that test.  Unselected rows may hold any target, and their logits are never loaded.
// Per-row arithmetic: that of k_cross_entropy (pp_dbgnn.hip) — (m - z[y]) + log1p(sum over c != argmax of exp(z[c] - m)), and
// -(sum of the other classes) / sum at the target column.
#include "pp_internal.h"

#include <math.h>

namespace pp {

struct MaskedSums {                      // the device result of pp_cross_entropy_masked_f32 (32 bytes)
    float num, den, mean, inv_den;       // sum w[y] nll, sum w[y], num / den, 1 / den (0 where nothing valid is selected)
    int64_t selected, out_of_range;
};

struct MaskedRaw {                       // the same sums BEFORE the rounding to fp32 (pp_cross_entropy_masked_sums_f32, 32 bytes): what a rank of a
    double num, den;                     // partitioned run adds to its peers' sums — fp32 sums of different ranks could not be added without a
    int64_t selected, out_of_range;      // second rounding
};

// the one place where sums become the result: pp_cross_entropy_masked_f32 (one process) and pp_masked_finish_f32 (sums of all ranks) share it
__device__ __forceinline__ MaskedSums finish_sums(double a, double b, int64_t s, int64_t o) {
    MaskedSums r;
    r.num = (float)a;
    r.den = (float)b;
    r.mean = (float)(a / b);                               // 0 / 0 = NaN on an empty selection, as F.cross_entropy's mean
    r.inv_den = s - o > 0 ? (float)(1.0 / b) : 0.f;          // ... whose gradient is all zero, not 0 * inf
    r.selected = s;
    r.out_of_range = o;
    return r;
}

__device__ __forceinline__ bool row_selected(const uint8_t* __restrict__ mask, const int64_t* __restrict__ target, int64_t i, int64_t ignore_index,
                                             int use_ignore, int64_t& y) {
    if (mask && mask[i] == 0) return false;
    y = target[i];
    return !(use_ignore && y == ignore_index);
}

// One lane per row, C <= kMaxC classes in registers; kFull: C == kMaxC (the row loads and stores have compile-time offsets).
// Grid-stride over the rows; per-workgroup partials (double, so that the order in which the workgroups' shares are cut shows only below
// fp32) go to part_* and are summed in a fixed order by k_masked_finish.
template <int kMaxC, bool kFull>
__global__ __launch_bounds__(kBlock) void k_cross_entropy_masked(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                const uint8_t* __restrict__ mask, const float* __restrict__ weight, int64_t n, int C_arg,
                                                                int64_t ignore_index, int use_ignore, double* __restrict__ part_num,
                                                                double* __restrict__ part_den, int64_t* __restrict__ part_sel,
                                                                int64_t* __restrict__ part_bad, float* __restrict__ dlogits) {
    __shared__ double s_num[kWavesPerBlock], s_den[kWavesPerBlock];
    __shared__ int s_sel[kWavesPerBlock], s_bad[kWavesPerBlock];
    const int C = kFull ? kMaxC : C_arg;
    float num = 0.f, den = 0.f;
    int sel = 0, bad = 0;                                      // (per lane: at most n / 2048 + 1 rows with a full grid, n / 2048 with a grid of 8)
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int64_t y = 0;
        const bool chosen = row_selected(mask, target, i, ignore_index, use_ignore, y);
        const bool valid = chosen && y >= 0 && y < C;
        sel += chosen ? 1 : 0;
        bad += (chosen && !valid) ? 1 : 0;
        if (!valid) {
            if (dlogits) {
#pragma unroll
                for (int c = 0; c < kMaxC; ++c)
                    if (c < C) dlogits[i * C + c] = 0.f;
            }
            continue;
        }
        const float w = weight ? weight[y] : 1.f;
        float z[kMaxC];
        float m = -INFINITY, zy = -INFINITY;
        int am = 0;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
            z[c] = c < C ? logits[i * C + c] : -INFINITY;
            if (c == y) zy = z[c];
            if (z[c] > m) { m = z[c]; am = c; }
        }
        float sum = 0.f, rest = 0.f, others = 0.f;            // all classes; all but the maximum's; all but the target's
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
            z[c] = c < C ? expf(z[c] - m) : 0.f;
            sum += z[c];
            rest += c == am ? 0.f : z[c];
            others += c == y ? 0.f : z[c];
        }
        const float scale = w / sum;
        if (dlogits) {
#pragma unroll
            for (int c = 0; c < kMaxC; ++c)
                if (c < C) dlogits[i * C + c] = (c == y ? -others : z[c]) * scale;
        }
        num += w * ((m - zy) + log1pf(rest));
        den += w;
    }
    const double wnum = wave_sum((double)num), wden = wave_sum((double)den);
    const int wsel = wave_sum(sel), wbad = wave_sum(bad);
    if (lane_id() == 0) {
        s_num[wave_id()] = wnum;
        s_den[wave_id()] = wden;
        s_sel[wave_id()] = wsel;
        s_bad[wave_id()] = wbad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        int64_t s = 0, o = 0;
#pragma unroll
        for (int wv = 0; wv < kWavesPerBlock; ++wv) {
            a += s_num[wv];
            b += s_den[wv];
            s += s_sel[wv];
            o += s_bad[wv];
        }
        part_num[blockIdx.x] = a;
        part_den[blockIdx.x] = b;
        part_sel[blockIdx.x] = s;
        part_bad[blockIdx.x] = o;
    }
}

// out = the sums of the n_parts per-workgroup partials in a fixed order (thread j takes j, j + 256, ..; fixed-shape tree over the threads)
__global__ __launch_bounds__(kBlock) void k_masked_finish(const double* __restrict__ part_num, const double* __restrict__ part_den,
                                                         const int64_t* __restrict__ part_sel, const int64_t* __restrict__ part_bad, int n_parts,
                                                         MaskedSums* __restrict__ out, MaskedRaw* __restrict__ raw) {
    __shared__ double s_num[kWavesPerBlock], s_den[kWavesPerBlock];
    __shared__ int64_t s_sel[kWavesPerBlock], s_bad[kWavesPerBlock];
    double a = 0.0, b = 0.0;
    int64_t s = 0, o = 0;
    for (int j = threadIdx.x; j < n_parts; j += kBlock) {
        a += part_num[j];
        b += part_den[j];
        s += part_sel[j];
        o += part_bad[j];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    s = wave_sum(s);
    o = wave_sum(o);
    if (lane_id() == 0) {
        s_num[wave_id()] = a;
        s_den[wave_id()] = b;
        s_sel[wave_id()] = s;
        s_bad[wave_id()] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0.0;
        s = o = 0;
#pragma unroll
        for (int wv = 0; wv < kWavesPerBlock; ++wv) {
            a += s_num[wv];
            b += s_den[wv];
            s += s_sel[wv];
            o += s_bad[wv];
        }
        if (out) *out = finish_sums(a, b, s, o);
        if (raw) *raw = MaskedRaw{a, b, s, o};
    }
}

// sums of all ranks (reduced by the caller) -> the result, with the arithmetic of k_masked_finish
__global__ void k_masked_finish_reduced(const double* __restrict__ sums, const int64_t* __restrict__ counts, MaskedSums* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = finish_sums(sums[0], sums[1], counts[0], counts[1]);
}

// counts[y][argmax z] += 1 over the selected rows: one lane per row, a per-workgroup histogram in LDS (C * C words: 16 KB at C = 64), its
// non-zero bins flushed with 64-bit integer atomics (sums of integers: the result does not depend on the order).  The prediction is the
// lowest column that holds the row maximum, a NaN counting as the maximum (numpy's argmax).  A workgroup's bin holds at most its share of
// the rows (n / 8 at the smallest grid), far below 2^31 for any [n, C] that fits the device.
template <int kMaxC>
__global__ __launch_bounds__(kBlock) void k_confusion(const float* __restrict__ logits, const int64_t* __restrict__ target, const uint8_t* __restrict__ mask,
                                                     int64_t n, int C, int64_t ignore_index, int use_ignore, unsigned long long* __restrict__ counts,
                                                     unsigned long long* __restrict__ status) {
    __shared__ unsigned int s_bins[kMaxC * kMaxC];
    for (int b = threadIdx.x; b < C * C; b += kBlock) s_bins[b] = 0u;
    __syncthreads();
    unsigned int bad = 0u;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        int64_t y = 0;
        if (!row_selected(mask, target, i, ignore_index, use_ignore, y)) continue;
        if (y < 0 || y >= C) { ++bad; continue; }
        float best = logits[i * C];
        int am = 0;
#pragma unroll
        for (int c = 1; c < kMaxC; ++c) {
            if (c < C) {
                const float v = logits[i * C + c];
                if (best == best && (v > best || v != v)) { best = v; am = c; }      // (once best is a NaN it stays)
            }
        }
        atomicAdd(&s_bins[(int)y * C + am], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < C * C; b += kBlock) {
        const unsigned int v = s_bins[b];
        if (v) atomicAdd(&counts[b], (unsigned long long)v);
    }
    bad = wave_sum(bad);
    if (lane_id() == 0 && bad) atomicAdd(status, (unsigned long long)bad);
}

// grid of a row-per-lane kernel: what is resident at once (asked from the runtime once per kernel) times the calling thread's launch
// share, never more than the rows provide
template <typename Kernel>
static int loss_blocks(Kernel kernel, int* resident, int64_t n, int64_t* blocks_out) {
    if (*resident == 0) {
        int per_cu = 0, dev = 0, cus = 0;
        PP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0));
        PP_HIP(hipGetDevice(&dev));
        PP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        *resident = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 256);
    }
    int64_t blocks = ceil_div(n, kBlock);
    const int64_t share = shared_grid(*resident);
    if (blocks > share) blocks = share;
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    note_persistent_grid(blocks);
    *blocks_out = blocks;
    return PP_OK;
}

struct MaskedParts {
    double *num, *den;
    int64_t *sel, *bad;
};

template <int kMaxC, bool kFull>
static int launch_masked(hipStream_t st, const float* logits, const int64_t* target, const uint8_t* mask, const float* weight, int64_t n, int C,
                         int64_t ignore_index, int use_ignore, MaskedParts p, float* dlogits, int64_t* blocks_out) {
    static int resident = 0;
    const int rc = loss_blocks(k_cross_entropy_masked<kMaxC, kFull>, &resident, n, blocks_out);
    if (rc != PP_OK) return rc;
    k_cross_entropy_masked<kMaxC, kFull><<<(unsigned)*blocks_out, kBlock, 0, st>>>(logits, target, mask, weight, n, C, ignore_index, use_ignore, p.num,
                                                                                 p.den, p.sel, p.bad, dlogits);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

template <int kMaxC>
static int launch_confusion(hipStream_t st, const float* logits, const int64_t* target, const uint8_t* mask, int64_t n, int C, int64_t ignore_index,
                            int use_ignore, int64_t* counts, int64_t* status) {
    static int resident = 0;
    int64_t blocks = 0;
    const int rc = loss_blocks(k_confusion<kMaxC>, &resident, n, &blocks);
    if (rc != PP_OK) return rc;
    k_confusion<kMaxC><<<(unsigned)blocks, kBlock, 0, st>>>(logits, target, mask, n, C, ignore_index, use_ignore, (unsigned long long*)counts,
                                                            (unsigned long long*)status);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

}  // namespace pp

extern "C" {

size_t pp_cross_entropy_masked_ws_bytes(void) { return 4 * pp::align_up((size_t)pp::kMaxGrid * sizeof(double)); }

static int masked_entry(const char* what, const float* logits, const int64_t* target, const uint8_t* mask, const float* weight, int64_t n, int C,
                        int64_t ignore_index, int use_ignore, pp::MaskedSums* result, pp::MaskedRaw* raw, float* dlogits_raw, void* ws, size_t ws_bytes,
                        hipStream_t st) {
    static_assert(sizeof(pp::MaskedSums) == 32, "the result is 4 floats and 2 int64");
    static_assert(sizeof(pp::MaskedRaw) == 32, "the raw sums are 2 doubles and 2 int64");
    PP_REQUIRE(n >= 0 && C >= 1 && C <= 64, PP_ERR_ARG, "%s: needs 1 <= C <= 64 (got %d)", what, C);
    PP_REQUIRE(ws != nullptr && ws_bytes >= pp_cross_entropy_masked_ws_bytes(), PP_ERR_WORKSPACE, "%s: workspace too small", what);
    pp::Arena arena(ws, ws_bytes);
    pp::MaskedParts p;
    p.num = arena.take<double>(pp::kMaxGrid);
    p.den = arena.take<double>(pp::kMaxGrid);
    p.sel = arena.take<int64_t>(pp::kMaxGrid);
    p.bad = arena.take<int64_t>(pp::kMaxGrid);
    int64_t blocks = 0;
    if (n > 0) {
        int rc;
        if (C == 8) rc = pp::launch_masked<8, true>(st, logits, target, mask, weight, n, C, ignore_index, use_ignore, p, dlogits_raw, &blocks);
        else if (C < 8) rc = pp::launch_masked<8, false>(st, logits, target, mask, weight, n, C, ignore_index, use_ignore, p, dlogits_raw, &blocks);
        else if (C == 16) rc = pp::launch_masked<16, true>(st, logits, target, mask, weight, n, C, ignore_index, use_ignore, p, dlogits_raw, &blocks);
        else if (C < 16) rc = pp::launch_masked<16, false>(st, logits, target, mask, weight, n, C, ignore_index, use_ignore, p, dlogits_raw, &blocks);
        else if (C == 64) rc = pp::launch_masked<64, true>(st, logits, target, mask, weight, n, C, ignore_index, use_ignore, p, dlogits_raw, &blocks);
        else rc = pp::launch_masked<64, false>(st, logits, target, mask, weight, n, C, ignore_index, use_ignore, p, dlogits_raw, &blocks);
        if (rc != PP_OK) return rc;
    }
    pp::k_masked_finish<<<1, pp::kBlock, 0, st>>>(p.num, p.den, p.sel, p.bad, (int)blocks, result, raw);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_cross_entropy_masked_f32(const float* logits, const int64_t* target, const uint8_t* mask, const float* weight, int64_t n, int C,
                                int64_t ignore_index, int use_ignore, void* result, float* dlogits_raw, void* ws, size_t ws_bytes, pp_stream_t stream) {
    PP_REQUIRE(result != nullptr && (uintptr_t)result % 8 == 0, PP_ERR_ARG, "pp_cross_entropy_masked_f32: result must be 32 bytes, 8-byte aligned");
    return masked_entry("pp_cross_entropy_masked_f32", logits, target, mask, weight, n, C, ignore_index, use_ignore, (pp::MaskedSums*)result, nullptr,
                        dlogits_raw, ws, ws_bytes, (hipStream_t)stream);
}

int pp_cross_entropy_masked_sums_f32(const float* logits, const int64_t* target, const uint8_t* mask, const float* weight, int64_t n, int C,
                                     int64_t ignore_index, int use_ignore, void* raw_sums, float* dlogits_raw, void* ws, size_t ws_bytes,
                                     pp_stream_t stream) {
    PP_REQUIRE(raw_sums != nullptr && (uintptr_t)raw_sums % 8 == 0, PP_ERR_ARG, "pp_cross_entropy_masked_sums_f32: raw_sums must be 32 bytes, 8-byte aligned");
    return masked_entry("pp_cross_entropy_masked_sums_f32", logits, target, mask, weight, n, C, ignore_index, use_ignore, nullptr,
                        (pp::MaskedRaw*)raw_sums, dlogits_raw, ws, ws_bytes, (hipStream_t)stream);
}

int pp_masked_finish_f32(const double* sums, const int64_t* counts, void* result, pp_stream_t stream) {
    PP_REQUIRE(sums != nullptr && counts != nullptr, PP_ERR_ARG, "pp_masked_finish_f32: sums [2] and counts [2] are required");
    PP_REQUIRE(result != nullptr && (uintptr_t)result % 8 == 0, PP_ERR_ARG, "pp_masked_finish_f32: result must be 32 bytes, 8-byte aligned");
    pp::k_masked_finish_reduced<<<1, 1, 0, (hipStream_t)stream>>>(sums, counts, (pp::MaskedSums*)result);
    PP_LAUNCH_CHECK();
    return PP_OK;
}

int pp_confusion_f32(const float* logits, const int64_t* target, const uint8_t* mask, int64_t n, int C, int64_t ignore_index, int use_ignore,
                     int64_t* counts, int64_t* status, pp_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    PP_REQUIRE(n >= 0 && C >= 1 && C <= 64, PP_ERR_ARG, "pp_confusion_f32: needs 1 <= C <= 64 (got %d)", C);
    PP_REQUIRE(counts != nullptr && status != nullptr, PP_ERR_ARG, "pp_confusion_f32: counts and status are required");
    PP_HIP(hipMemsetAsync(counts, 0, (size_t)C * C * sizeof(int64_t), st));
    PP_HIP(hipMemsetAsync(status, 0, sizeof(int64_t), st));
    if (n == 0) return PP_OK;
    if (C <= 8) return pp::launch_confusion<8>(st, logits, target, mask, n, C, ignore_index, use_ignore, counts, status);
    if (C <= 16) return pp::launch_confusion<16>(st, logits, target, mask, n, C, ignore_index, use_ignore, counts, status);
    return pp::launch_confusion<64>(st, logits, target, mask, n, C, ignore_index, use_ignore, counts, status);
}

}  // extern "C"
