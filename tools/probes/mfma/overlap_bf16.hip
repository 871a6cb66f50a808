// Does a SIMD overlap one wave's bf16 MFMA burst with another wave's VALU work?  The shape of overlap.hip (whose fp32 MFMAs do NOT overlap with
// VALU): 512-thread workgroups, waves 0-3 (one per SIMD) run v_mfma_f32_16x16x32_bf16 with B from LDS (one ds_read_b128 per operand, 4 MFMAs
// per read), waves 4-7 run the same dependency-free FMA loop.  Times: MFMA only, VALU only, both.
//   hipcc -O3 --offload-arch=gfx950 overlap_bf16.hip -o overlap_bf16 && ./overlap_bf16
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16;
constexpr int kFrags = 64;                                 // B operands in LDS: [frag][lane] x 8 bf16, 64 KB

__global__ __launch_bounds__(512) void k_both(const uint4* __restrict__ W, int tiles, int do_mfma, int do_valu, float* __restrict__ out) {
    __shared__ uint4 s_w[kFrags * 64];
    for (int e = threadIdx.x; e < kFrags * 64; e += 512) s_w[e] = W[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 4) {
        if (!do_mfma) return;
        uint4 a[4];
        for (int c = 0; c < 4; ++c) a[c] = make_uint4(0x3f803f80u + lane, 0x3f803f80u + c, 0x3f803f80u, 0x3f803f80u);
        f32x4 total = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < tiles; ++t) {
#pragma unroll 1
            for (int chunk = 0; chunk < 16; ++chunk) {                   // 16 chunks x 32 MFMAs = 512 MFMAs per "tile" (16 cycles each: the 8192 cycles of overlap.hip)
                uint4 b[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) b[c] = s_w[((chunk & (kFrags / 8 - 1)) * 8 + c) * 64 + lane];
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int rep = 0; rep < 4; ++rep)
#pragma unroll
                    for (int c = 0; c < 8; c += 2) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[rep]), __builtin_bit_cast(bf16x8, b[c]), acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[rep]), __builtin_bit_cast(bf16x8, b[c + 1]), acc1, 0, 0, 0);
                    }
                total += acc0 + acc1;
            }
        }
        if (total[0] == 12345.678f) out[threadIdx.x] = total[1];
    } else {
        if (!do_valu) return;
        float x0 = lane, x1 = lane + 1, x2 = lane + 2, x3 = lane + 3, x4 = 1.f, x5 = 2.f, x6 = 3.f, x7 = 4.f;
        for (int it = 0; it < tiles * 136; ++it) {         // 8 FMAs per iteration: ~1090 VALU per "tile", as in overlap.hip
            x0 = x0 * 1.0001f + 0.5f; x1 = x1 * 1.0001f + 0.5f; x2 = x2 * 1.0001f + 0.5f; x3 = x3 * 1.0001f + 0.5f;
            x4 = x4 * 1.0001f + 0.5f; x5 = x5 * 1.0001f + 0.5f; x6 = x6 * 1.0001f + 0.5f; x7 = x7 * 1.0001f + 0.5f;
        }
        if (x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7 == 1.2345f) out[threadIdx.x] = x0;
    }
}

int main() {
    const int blocks = 256, tiles = 600;
    uint4* w; float* out;
    hipMalloc(&w, kFrags * 64 * sizeof(uint4)); hipMalloc(&out, 4096);
    std::vector<uint32_t> h(kFrags * 64 * 4, 0x3f003f00u);             // bf16 0.5 everywhere
    hipMemcpy(w, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const char* names[3] = {"MFMA only", "VALU only", "MFMA + VALU"};
    for (int rep = 0; rep < 2; ++rep)
        for (int mode = 0; mode < 3; ++mode) {
            hipEventRecord(e0);
            k_both<<<blocks, 512>>>(w, tiles, mode != 1, mode != 0, out);
            hipEventRecord(e1); hipEventSynchronize(e1);
            float ms = 0; hipEventElapsedTime(&ms, e0, e1);
            if (rep) printf("%-12s %7.3f ms\n", names[mode], ms);
        }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
