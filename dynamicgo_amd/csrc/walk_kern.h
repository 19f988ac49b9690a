/*
 * walk_kern.h — the lane pass and the deep pass of every component that walks
 * (item, k) pairs with tget_device.h's frames: tget, the cols, ents and rows
 * cell passes and the rows head and index passes (one "column" per message).
 * Included by the *_kern.hip units only: the *_device.h headers are also built
 * for the host and hold no __global__ code.
 *
 * The protocol, once. The lane pass gives a lane one pair and walks it with
 * TG_LDS_DEPTH frames in LDS; a pair that nests deeper is queued
 * (atomicAdd(count)) and nothing of it is stored. The deep pass, launched
 * behind it on the same stream, strides over the queue with TG_DEEP_LANES lanes
 * and TG_DEEP_DEPTH frames per lane in device memory and walks each queued pair
 * again from the start. It also zeroes the other counter, the one the previous
 * launch used (AltCounters, host_internal.h): no launch pays a memset.
 *
 * An operation OP names
 *   Params, Lds, Deep   the parameter struct and the two frame types;
 *   pairs(A)            how many pairs there are (read on the device where the
 *                       host does not know it);
 *   queue(A)            where the queue, this pass's counter, the other counter
 *                       and the deep frames live (WalkQueue);
 *   lane<FR>(A, q, fr)  pair q walked with the LDS frames and stored. true: it
 *                       needs the deep frames and nothing was stored;
 *   deep<FR>(A, q, fr)  pair q walked with the deep frames and stored. There
 *                       is no deeper pass: the operation stores what it stores
 *                       for a pair that still answers deep (unreachable: 1023
 *                       levels fit). Its answer, if it has one, is unused.
 * Both are called as OP::template lane<FR>(...), so an operation whose walk is
 * one existing function names it by pointer (a static constexpr variable
 * template) and the kernel calls that function itself, as the kernel it
 * replaces did. A forwarding function there is one more inlined layer, which
 * changed the code the compiler generates for the walk inside it (rows' head
 * pass: 7 165 instructions against 7 160) and measured 1 % slower on long lists.
 *
 * The kids lane and deep kernels (kids_kern.hip) stay their own: the wide queue,
 * two counters per set, the stats counter and their own block and frame
 * constants would each be one more parameter here and remove no code there.
 */
#pragma once
#include "tget_device.h"

namespace dg {

struct WalkQueue {
    uint32_t *list;  /* pairs queued for the deep pass */
    uint32_t *count; /* this pass's counter */
    uint32_t *reset; /* the other one, zeroed by the deep pass */
    uint64_t *ws;    /* deep frames: [level * TG_DEEP_LANES + lane] */
};
static __device__ __forceinline__ WalkQueue walk_queue(const TGParams &T)
{
    return WalkQueue{T.deep_list, T.deep_count, T.reset_count, T.ws};
}

/* Every SP-th lane takes one pair; neighbouring pairs sit in neighbouring
 * lanes. SP is tget's lane spacing (tget_kern.hip), 1 everywhere else. */
template <class OP, uint32_t SP = 1>
__global__ __launch_bounds__(TG_BLOCK) void walk_pass_kernel(typename OP::Params A)
{
    __shared__ uint64_t lf[TG_LDS_DEPTH * TG_BLOCK];
    if (threadIdx.x % SP) return;
    const uint64_t q = ((uint64_t)blockIdx.x * TG_BLOCK + threadIdx.x) / SP;
    if (q >= OP::pairs(A)) return;
    const typename OP::Lds fr{&lf[threadIdx.x]};
    if (OP::template lane<typename OP::Lds>(A, q, fr)) {
        const WalkQueue Q = OP::queue(A);
        Q.list[atomicAdd(Q.count, 1u)] = (uint32_t)q;
    }
}

/* the queued pairs again from the start; a small grid striding over the queue
 * (deep values are rare). Also zeroes the counter the previous launch used. */
template <class OP>
__global__ __launch_bounds__(TG_DEEP_BLOCK) void walk_deep_kernel(typename OP::Params A)
{
    const WalkQueue Q = OP::queue(A);
    const uint32_t cnt = *(volatile const uint32_t *)Q.count;
    const uint32_t lane = blockIdx.x * TG_DEEP_BLOCK + threadIdx.x;
    if (lane == 0) *Q.reset = 0;
    const typename OP::Deep fr{Q.ws + lane};
    for (uint32_t g = lane; g < cnt; g += TG_DEEP_LANES) (void)OP::template deep<typename OP::Deep>(A, Q.list[g], fr);
}

/* the lane pass over `pairs` pairs and its deep pass behind it */
template <class OP>
static inline void launch_walk(hipStream_t s, const typename OP::Params &A, uint64_t pairs)
{
    hipLaunchKernelGGL((walk_pass_kernel<OP, 1>), dim3((uint32_t)((pairs + TG_BLOCK - 1) / TG_BLOCK)), dim3(TG_BLOCK), 0, s, A);
    hipLaunchKernelGGL(walk_deep_kernel<OP>, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

}  // namespace dg
