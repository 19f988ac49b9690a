/* edit kernels (batched SetMany, and SetByPath / UnsetByPath as its K = 1;
 * editm_device.h): the splice's lane route and wave route, instantiated per
 * item count K = 1..7 so that the segment table of K cuts is indexed by
 * constants only and stays in registers. Both read the lookup's K + 1 records
 * per message, take the same decision and leave a message to the other kernel
 * when its output length puts it there (EmParams::wave_min), so no queue is
 * needed: the decision costs K + 1 16-byte records and at most one 16-byte
 * window of the message per item. */
#include "editm_device.h"

namespace dg {

/* G lanes per message (1, 4 or 16) take the aligned 16-byte units of its output
 * in turn, so G neighbouring lanes store G x 16 contiguous bytes; with G = 1 a
 * lane assembles and stores every unit of its message itself */
template <uint32_t KT, uint32_t G>
__global__ __launch_bounds__(ED_BLOCK) void editm_lane_kernel(EmParams A)
{
    const uint64_t i = ((uint64_t)blockIdx.x * ED_BLOCK + threadIdx.x) / G;
    if (i >= A.n) return;
    editm_message<KT, G, false>(A, i, threadIdx.x % G);
}

/* one wave per message, a fixed grid striding over the batch: the 64 lanes take
 * the output's aligned 16-byte units in turn, so a wave's stores are one
 * contiguous KiB; the message index comes from readfirstlane: the records, the
 * decision and the table are wave-uniform */
template <uint32_t KT>
__global__ __launch_bounds__(ED_WAVES * 64) void editm_wave_kernel(EmParams A)
{
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * ED_WAVES + wv; i < A.n; i += (uint64_t)gridDim.x * ED_WAVES)
        editm_message<KT, 64, true>(A, i, lane);
}

template <uint32_t KT>
static void lane_k(hipStream_t s, const EmParams &A, uint32_t lanes)
{
    const dim3 grid((uint32_t)((A.n * lanes + ED_BLOCK - 1) / ED_BLOCK)), block(ED_BLOCK);
    if (lanes == 16) hipLaunchKernelGGL((editm_lane_kernel<KT, 16>), grid, block, 0, s, A);
    else if (lanes == 4) hipLaunchKernelGGL((editm_lane_kernel<KT, 4>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((editm_lane_kernel<KT, 1>), grid, block, 0, s, A);
}

template <uint32_t KT>
static void wave_k(hipStream_t s, const EmParams &A, uint32_t blocks)
{
    hipLaunchKernelGGL((editm_wave_kernel<KT>), dim3(blocks), dim3(ED_WAVES * 64), 0, s, A);
}

#define EM_BY_K(fn, ...)                                 \
    switch (A.K) {                                       \
        case 1: fn<1>(__VA_ARGS__); break;               \
        case 2: fn<2>(__VA_ARGS__); break;               \
        case 3: fn<3>(__VA_ARGS__); break;               \
        case 4: fn<4>(__VA_ARGS__); break;               \
        case 5: fn<5>(__VA_ARGS__); break;               \
        case 6: fn<6>(__VA_ARGS__); break;               \
        case 7: fn<7>(__VA_ARGS__); break;               \
        default: break; /* dg_editm_create lets 1..7 through */ \
    }

void launch_editm_lane(hipStream_t s, const EmParams &A, uint32_t lanes) { EM_BY_K(lane_k, s, A, lanes) }

void launch_editm_wave(hipStream_t s, const EmParams &A, uint32_t blocks) { EM_BY_K(wave_k, s, A, blocks) }

}  // namespace dg
