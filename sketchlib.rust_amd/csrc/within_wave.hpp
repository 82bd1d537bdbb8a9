// within_wave.hpp -- how ONE WAVE reads its span of a dense band and finds the positions that pass the cap (device code, wave64):
// the 16-byte loads and the ballots that within.hip's count and scatter kernels, cluster.hip's union kernel and mst.hip's
// min-edge kernel share.  The chunking, the cap predicate and the (i, j) of a position are within_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include "within_plan.hpp"

namespace skl {

__device__ __forceinline__ uint32_t within_lanes_below(uint64_t m)   // set bits of m below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// A wave's trips over its span of a chunk, from position w0 of a band of m positions ([m][NCOLS] f32, 16-byte aligned,
// within_band_bytes(m, NCOLS) readable): the 16-byte loads and, per element of a load, the ballot of the lanes whose position
// exists and passes.  Returns the wave's total.
template <uint32_t NCOLS>
struct WithinWave {
    static constexpr uint32_t V = NCOLS == 2u ? 2u : 4u;                 // positions per load: V * NCOLS = 4 floats
    static constexpr uint32_t TRIPS = WITHIN_WAVE_SPAN / (64u * V);
    float4 v[TRIPS];
    uint64_t pass[TRIPS][V];

    __device__ __forceinline__ uint32_t load(const float *__restrict__ band, uint64_t m, const WithinPred &pred, uint64_t w0, uint32_t lane)
    {
        return load_if(band, m, w0, lane, [&pred](float v0, float v1) { return within_keep(pred, v0, v1); });
    }
    // ... with any predicate keep(v0, v1) on the two stored values of a position (v1 = 0 with one column): mst.hip's is its own
    template <typename Keep>
    __device__ __forceinline__ uint32_t load_if(const float *__restrict__ band, uint64_t m, uint64_t w0, uint32_t lane, Keep keep_of)
    {
        const float4 *__restrict__ src = reinterpret_cast<const float4 *>(band);
        uint32_t total = 0;
#pragma unroll
        for (uint32_t t = 0; t < TRIPS; ++t) {
            const uint64_t p = w0 + (uint64_t)(t * 64u + lane) * V;
            v[t] = src[p < m ? p / V : 0u];   // (unconditional: it stays one 16-byte load; position 0 exists)
            const float f[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
#pragma unroll
            for (uint32_t e = 0; e < V; ++e) {
                const bool keep = p + e < m && keep_of(f[e * NCOLS], NCOLS == 2u ? f[e * NCOLS + 1u] : 0.0f);
                pass[t][e] = __ballot(keep);
                total += (uint32_t)__popcll(pass[t][e]);
            }
        }
        return total;
    }
};

}  // namespace skl
