// pathpyg_amd — the Philox4x32-10 word shared by the samplers (pp_random_graphs.hip, pp_graph_layout.hip).
#pragma once
#include "pp_common.h"

namespace pp {

// One block of Philox4x32-10 (Salmon et al., Random123) keyed by (k0, k1); counter c0, c1 = index, c2 = the low 32 bits of `stream`,
// c3 = tag << 24 | stream bits 32 .. 55.  Returns x | y << 32.  Every use owns a tag (PP_RG_TAG_*), so no two uses share a counter.
__device__ __forceinline__ uint64_t rg_word(uint32_t k0, uint32_t k1, uint32_t tag, uint64_t stream, uint64_t index) {
    uint32_t c0 = (uint32_t)index, c1 = (uint32_t)(index >> 32), c2 = (uint32_t)stream, c3 = (tag << 24) | ((uint32_t)(stream >> 32) & 0xFFFFFFu);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (uint64_t)c0 | ((uint64_t)c1 << 32);
}

}  // namespace pp
