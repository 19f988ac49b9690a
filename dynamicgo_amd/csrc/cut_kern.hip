/* cut kernels (batched MarshalTo, cut_device.h): the lane route and the wave route. */
#include "cut_device.h"

namespace dg {

/* The walk reads the plan at every field (the node, a binary search of its
 * fields, the child's node): dependent loads on the critical path. The lane
 * route copies a plan whose tables fit CAP bytes to LDS first (the literal
 * pool stays in device memory: it is read only at a STOP with unset fields,
 * 16 unaligned bytes at a time). Measured on ~1 KB messages: 204 -> 226 GB/s.
 * The wave route, whose plan loads are wave-uniform, lost by it (26 -> 17
 * GB/s) and reads the plan where it is. */
template <uint32_t CAP>
__device__ __forceinline__ CutPlanView cut_stage_plan(const CutParams &A, uint8_t *lds)
{
    CutPlanView P = A.plan;
    if (A.tab_len > CAP) return P; /* the same for every thread */
    for (uint32_t q = threadIdx.x * 8; q < A.tab_len; q += blockDim.x * 8) /* tab_len is a multiple of 8 */
        *(uint64_t *)(void *)(lds + q) = *(const uint64_t *)(const void *)(A.blob + q);
    __syncthreads();
    P.nodes = (const dg_cut_node *)(const void *)(lds + A.off_nodes);
    P.fields = (const dg_cut_field *)(const void *)(lds + A.off_fields);
    P.lits = (const dg_cut_lit *)(const void *)(lds + A.off_lits);
    return P;
}
constexpr uint32_t CUT_LANE_PLAN = 5120;  /* with the frames 53 KB a block: three blocks a CU still */

/* One lane per message: 8 cut frames and 8 skip frames per lane in LDS, the
 * kept runs copied by the lane itself (CutLaneSink). A message at least
 * wave_min bytes long, or one that opens more frames than these, is queued for
 * cut_wave_kernel (what the lane wrote before it declined lies inside the
 * message's own slot and is written again). */
__global__ __launch_bounds__(CUT_BLOCK) void cut_lane_kernel(CutParams A)
{
    __shared__ uint64_t meta[CUT_LDS_DEPTH * CUT_BLOCK], mask[CUT_LDS_DEPTH * CUT_BLOCK];
    __shared__ uint64_t skf[TG_LDS_DEPTH * TG_BLOCK];
    static_assert(TG_BLOCK == CUT_BLOCK, "the skip frames are strided by tget's block");
    __shared__ __attribute__((aligned(16))) uint8_t plan[CUT_LANE_PLAN];
    const CutPlanView P = cut_stage_plan<CUT_LANE_PLAN>(A, plan);
    const uint64_t i = (uint64_t)blockIdx.x * CUT_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t a = A.in_off[i], len = A.in_off[i + 1] - a;
    CutRes r{CUT_ST_DEEP, 0};
    CutLaneSink sk{A.out + A.out_off[i], A.out_off[i + 1] - A.out_off[i], 0, false};
    if (len < A.wave_min) {
        const CutLdsFrames fr{&meta[threadIdx.x], &mask[threadIdx.x]};
        const TGLdsFrames sf{&skf[threadIdx.x]};
        r = cut_walk(P, A.opts, A.src + a, len, fr, sf, sk);
    }
    if (r.status == CUT_ST_DEEP || r.status == CUT_ST_SKIPDEEP) {
        A.wave_list[atomicAdd(A.wave_count, 1u)] = (uint32_t)i;
        return;
    }
    cut_store(A, i, r, sk.o, sk.ovf);
}

/* One wave per queued message, a fixed grid striding over the queue. Every
 * lane runs the same walk on the same addresses (the message index comes from
 * readfirstlane, so the compiler sees them wave-uniform); the frames, 64 cut
 * and 1024 skip frames per wave, sit in LDS and every lane stores the same
 * words there. The 64 lanes share each copy (CutWaveSink). Also zeroes the
 * counter the previous launch used. */
__global__ __launch_bounds__(CUT_WAVES * 64) void cut_wave_kernel(CutParams A)
{
    __shared__ uint64_t meta[CUT_WAVES * DG_CUT_MAX_DEPTH], mask[CUT_WAVES * DG_CUT_MAX_DEPTH];
    __shared__ uint64_t skf[CUT_WAVES * TG_DEEP_DEPTH];
    const CutPlanView P = A.plan; /* wave-uniform loads from device memory; staged in LDS they measured slower */
    const uint32_t cnt = *(volatile const uint32_t *)A.wave_count;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.reset_count = 0;
    const CutWaveFrames fr{&meta[wv * DG_CUT_MAX_DEPTH], &mask[wv * DG_CUT_MAX_DEPTH]};
    const CutWaveSkipFrames sf{&skf[wv * TG_DEEP_DEPTH]};
    for (uint32_t g = blockIdx.x * CUT_WAVES + wv; g < cnt; g += gridDim.x * CUT_WAVES) {
        const uint64_t i = A.wave_list[g];
        const uint64_t a = A.in_off[i], len = A.in_off[i + 1] - a;
        CutWaveSink sk{A.out + A.out_off[i], A.out_off[i + 1] - A.out_off[i], 0, false, lane};
        CutRes r = cut_walk(P, A.opts, A.src + a, len, fr, sf, sk);
        if (r.status == CUT_ST_DEEP) r = CutRes{DG_CUT_E_DEPTH, 0};
        if (r.status == CUT_ST_SKIPDEEP) r = CutRes{DG_CUT_E_READ, 0}; /* unreachable: 1023 levels fit */
        if (lane == 0) cut_store(A, i, r, sk.o, sk.ovf);
    }
}

void launch_cut_lane(hipStream_t s, const CutParams &A)
{
    hipLaunchKernelGGL(cut_lane_kernel, dim3((uint32_t)((A.n + CUT_BLOCK - 1) / CUT_BLOCK)), dim3(CUT_BLOCK), 0, s, A);
}

void launch_cut_wave(hipStream_t s, const CutParams &A, uint32_t blocks)
{
    hipLaunchKernelGGL(cut_wave_kernel, dim3(blocks), dim3(CUT_WAVES * 64), 0, s, A);
}

}  // namespace dg
