/* tget kernels (batched GetByPath, tget_device.h): the pair pass (walk_kern.h) over (message, path) pairs. */
#include "walk_kern.h"

namespace dg {

/* Pair q = (message q / P, path q % P): the P pairs of a message sit in
 * neighbouring lanes and read the same lines. The walk is a chain of dependent
 * loads like the t2j lane pass's, but sparser waves (SP 2, 4), which pay there,
 * measured no faster here: the host launches SP 1 unless the tget_spread knob
 * says otherwise (tget_host.hip). */
struct TgetOp {
    using Params = TGParams;
    using Lds = TGLdsFrames;
    using Deep = TGDeepFrames;
    static __device__ __forceinline__ uint64_t pairs(const TGParams &A) { return A.pairs; }
    static __device__ __forceinline__ WalkQueue queue(const TGParams &A) { return walk_queue(A); }
    template <class FR>
    static __device__ __forceinline__ bool pair(const TGParams &A, uint64_t q, const FR &fr, bool last)
    {
        const uint64_t i = q / A.P;
        const uint32_t k = (uint32_t)(q - i * A.P);
        const uint64_t a = A.in_off[i], e = A.in_off[i + 1];
        TGRes r = tg_walk(A, A.src + a, e - a, k, fr);
        if (r.status == TG_ST_DEEP) {
            if (!last) return true;
            r = tg_res(DG_TGET_E_READ, r.step); /* unreachable: 1023 levels fit */
        }
        tg_store(A, q, a, r);
        return false;
    }
    template <class FR>
    static __device__ __forceinline__ bool lane(const TGParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, false); }
    template <class FR>
    static __device__ __forceinline__ bool deep(const TGParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, true); }
};

void launch_tget_pass(hipStream_t s, const TGParams &A, uint32_t spread)
{
    const uint64_t lanes = A.pairs * spread;
    const dim3 grid((uint32_t)((lanes + TG_BLOCK - 1) / TG_BLOCK)), block(TG_BLOCK);
    if (spread == 1) hipLaunchKernelGGL((walk_pass_kernel<TgetOp, 1>), grid, block, 0, s, A);
    else if (spread == 4) hipLaunchKernelGGL((walk_pass_kernel<TgetOp, 4>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((walk_pass_kernel<TgetOp, 2>), grid, block, 0, s, A);
}

void launch_tget_deep(hipStream_t s, const TGParams &A)
{
    hipLaunchKernelGGL(walk_deep_kernel<TgetOp>, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

}  // namespace dg
