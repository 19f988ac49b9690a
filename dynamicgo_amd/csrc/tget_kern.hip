/* tget kernels (batched GetByPath, tget_device.h): the LDS-frame pass and the deep pass. */
#include "tget_device.h"

namespace dg {

/* Every SP-th lane takes one (message, path) pair; the P pairs of a message
 * sit in neighbouring lanes and read the same lines. The walk is a chain of
 * dependent loads like the t2j lane pass's, but sparser waves (SP 2, 4), which
 * pay there, measured no faster here: the host launches SP 1 unless the
 * tget_spread knob says otherwise (tget_host.hip). Pairs whose skip nests
 * beyond the LDS frames are queued for tget_deep_kernel. */
template <uint32_t SP>
__global__ __launch_bounds__(TG_BLOCK) void tget_kernel(TGParams A)
{
    __shared__ uint64_t lf[TG_LDS_DEPTH * TG_BLOCK];
    if (threadIdx.x % SP) return;
    const uint64_t q = ((uint64_t)blockIdx.x * TG_BLOCK + threadIdx.x) / SP;
    if (q >= A.pairs) return;
    const uint64_t i = q / A.P;
    const uint32_t k = (uint32_t)(q - i * A.P);
    const uint64_t a = A.in_off[i], e = A.in_off[i + 1];
    const TGLdsFrames fr{&lf[threadIdx.x]};
    const TGRes r = tg_walk(A, A.src + a, e - a, k, fr);
    if (r.status == TG_ST_DEEP) {
        A.deep_list[atomicAdd(A.deep_count, 1u)] = (uint32_t)q;
        return;
    }
    tg_store(A, q, a, r);
}

/* the queued pairs again from the start, TG_DEEP_DEPTH frames per lane in
 * device memory; a small grid striding over the queue (deep values are rare).
 * Also zeroes the counter the previous launch used. */
__global__ __launch_bounds__(TG_DEEP_BLOCK) void tget_deep_kernel(TGParams A)
{
    const uint32_t cnt = *(volatile const uint32_t *)A.deep_count;
    const uint32_t lane = blockIdx.x * TG_DEEP_BLOCK + threadIdx.x;
    if (lane == 0) *A.reset_count = 0;
    const TGDeepFrames fr{A.ws + lane};
    for (uint32_t g = lane; g < cnt; g += TG_DEEP_LANES) {
        const uint64_t q = A.deep_list[g];
        const uint64_t i = q / A.P;
        const uint32_t k = (uint32_t)(q - i * A.P);
        const uint64_t a = A.in_off[i], e = A.in_off[i + 1];
        TGRes r = tg_walk(A, A.src + a, e - a, k, fr);
        if (r.status == TG_ST_DEEP) r = tg_res(DG_TGET_E_READ, r.step); /* unreachable: 1023 levels fit */
        tg_store(A, q, a, r);
    }
}

void launch_tget_pass(hipStream_t s, const TGParams &A, uint32_t spread)
{
    const uint64_t lanes = A.pairs * spread;
    const dim3 grid((uint32_t)((lanes + TG_BLOCK - 1) / TG_BLOCK)), block(TG_BLOCK);
    if (spread == 1) hipLaunchKernelGGL(tget_kernel<1>, grid, block, 0, s, A);
    else if (spread == 4) hipLaunchKernelGGL(tget_kernel<4>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(tget_kernel<2>, grid, block, 0, s, A);
}

void launch_tget_deep(hipStream_t s, const TGParams &A)
{
    hipLaunchKernelGGL(tget_deep_kernel, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

}  // namespace dg
