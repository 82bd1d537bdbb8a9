// slab_ops.hip -- new row slabs from resident ones (skl_sketches_select; gfx950): a gather of whole sample rows.
//
// A sample's row in the reference layout is nk * sketchsize64 * 14 u64 = row_vec 16-byte words, contiguous, and the
// rows of a slab follow each other without padding: the copy is dst[r][c] = src[ids[r]][c] over uint4 words, one
// global_load_dwordx4 / global_store_dwordx4 per lane.  L = the power of two >= row_vec (8 .. 256) adjacent lanes walk
// one row together, so a wave-instruction touches L * 16 contiguous bytes of one source row (rows of 1 KiB and more:
// the full 1 KiB per instruction) and consecutive destination rows are contiguous in memory; a 256-thread workgroup
// carries 256 / L rows side by side.  A lane works on four rows at a time (a grid sweep apart) and issues their four loads
// before the first store, and the grid holds up to 16 workgroups per CU: with nothing to compute, access width and bytes
// in flight are all there is.  Every offset is 64-bit (a slab
// of a million five-k samples is 18 GB).
#include "kernels.h"

namespace skl {

constexpr int SG_THREADS = 256;
constexpr int SG_UNROLL = 4;
constexpr int SG_WG_PER_CU = 16;

__global__ __launch_bounds__(SG_THREADS) void slab_gather_kernel(const SlabGatherArgs a, const uint32_t lane_shift)
{
    const uint32_t lanes = 1u << lane_shift;                 // lanes per row
    const uint32_t rows_per_pass = SG_THREADS >> lane_shift; // rows a workgroup carries side by side
    const uint64_t sub = threadIdx.x >> lane_shift;
    const uint64_t col0 = threadIdx.x & (lanes - 1u);
    const uint64_t stride = (uint64_t)gridDim.x * rows_per_pass;
    const uint64_t last = a.n_ids - 1;   // (n_ids >= 1: launch_slab_gather)
    // SG_UNROLL rows per lane and trip, a grid sweep apart: their loads are all issued before the first store.  A row past the
    // end is read as the last row (a valid address, no branch among the loads) and not stored.
    static_assert(SG_UNROLL == 4, "the four rows of a trip are spelled out (arrays of them end up in LDS)");
    for (uint64_t r = (uint64_t)blockIdx.x * rows_per_pass + sub; r < a.n_ids; r += stride * SG_UNROLL) {
        const uint64_t r1 = r + stride, r2 = r + 2 * stride, r3 = r + 3 * stride;
        const bool live1 = r1 < a.n_ids, live2 = r2 < a.n_ids, live3 = r3 < a.n_ids;
        const uint64_t q1 = live1 ? r1 : last, q2 = live2 ? r2 : last, q3 = live3 ? r3 : last;
        const uint32_t i0 = a.ids[r], i1 = a.ids[q1], i2 = a.ids[q2], i3 = a.ids[q3];
        const uint4 *src0 = a.src + (uint64_t)i0 * a.row_vec, *src1 = a.src + (uint64_t)i1 * a.row_vec;
        const uint4 *src2 = a.src + (uint64_t)i2 * a.row_vec, *src3 = a.src + (uint64_t)i3 * a.row_vec;
        uint4 *dst0 = a.dst + r * a.row_vec, *dst1 = a.dst + q1 * a.row_vec, *dst2 = a.dst + q2 * a.row_vec, *dst3 = a.dst + q3 * a.row_vec;
        for (uint64_t c = col0; c < a.row_vec; c += lanes) {
            const uint4 v0 = src0[c], v1 = src1[c], v2 = src2[c], v3 = src3[c];
            dst0[c] = v0;
            if (live1) dst1[c] = v1;
            if (live2) dst2[c] = v2;
            if (live3) dst3[c] = v3;
        }
    }
}

hipError_t launch_slab_gather(const SlabGatherArgs &a, int n_cu, hipStream_t stream)
{
    if (a.n_ids == 0 || a.row_vec == 0) return hipSuccess;
    uint32_t lane_shift = 3;   // 8 lanes: the shortest row (one k-mer length, 64 bins) is 7 words
    while (lane_shift < 8 && (1ull << lane_shift) < a.row_vec) ++lane_shift;
    const uint64_t rows_per_pass = SG_THREADS >> lane_shift;
    const uint64_t passes = (a.n_ids + rows_per_pass - 1) / rows_per_pass;
    const uint64_t cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * SG_WG_PER_CU;
    const uint32_t grid = (uint32_t)(passes < cap ? passes : cap);
    hipLaunchKernelGGL(slab_gather_kernel, dim3(grid), dim3(SG_THREADS), 0, stream, a, lane_shift);
    return hipGetLastError();
}

}  // namespace skl
