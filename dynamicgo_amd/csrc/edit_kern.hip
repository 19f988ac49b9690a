/* edit kernels (batched SetByPath / UnsetByPath, edit_device.h): the splice's
 * lane route and wave route. Both read the lookup's records, take the same
 * decision per message and leave a message to the other kernel when its output
 * length puts it there (EditParams::wave_min), so no queue is needed: the
 * decision costs two 16-byte records and at most one 16-byte window of the
 * message. */
#include "edit_device.h"

namespace dg {

/* G lanes per message (1, 4 or 16): the G lanes take the aligned 16-byte units
 * of the message's output in turn, so G neighbouring lanes store G x 16
 * contiguous bytes; with G = 1 a lane assembles and stores every unit of its
 * message itself. */
template <uint32_t G>
__global__ __launch_bounds__(ED_BLOCK) void edit_lane_kernel(EditParams A)
{
    const uint64_t i = ((uint64_t)blockIdx.x * ED_BLOCK + threadIdx.x) / G;
    if (i >= A.n) return;
    edit_message<G, false>(A, i, threadIdx.x % G);
}

/* One wave per message, a fixed grid striding over the batch: the 64 lanes
 * take the output's aligned 16-byte units in turn, so a wave's stores are one
 * contiguous KiB. The message index comes from readfirstlane: the records and
 * the decision are wave-uniform. */
__global__ __launch_bounds__(ED_WAVES * 64) void edit_wave_kernel(EditParams A)
{
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * ED_WAVES + wv; i < A.n; i += (uint64_t)gridDim.x * ED_WAVES)
        edit_message<64, true>(A, i, lane);
}

void launch_edit_lane(hipStream_t s, const EditParams &A, uint32_t lanes)
{
    const dim3 grid((uint32_t)((A.n * lanes + ED_BLOCK - 1) / ED_BLOCK)), block(ED_BLOCK);
    if (lanes == 16) hipLaunchKernelGGL(edit_lane_kernel<16>, grid, block, 0, s, A);
    else if (lanes == 4) hipLaunchKernelGGL(edit_lane_kernel<4>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(edit_lane_kernel<1>, grid, block, 0, s, A);
}

void launch_edit_wave(hipStream_t s, const EditParams &A, uint32_t blocks)
{
    hipLaunchKernelGGL(edit_wave_kernel, dim3(blocks), dim3(ED_WAVES * 64), 0, s, A);
}

}  // namespace dg
