/* cols kernels (typed column reads, cols_device.h): the cell pass (walk_kern.h),
 * the scan of a list column's counts (scan_kern.h) and the element-parallel emit. */
#include "cols_device.h"
#include "scan_kern.h"
#include "walk_kern.h"

namespace dg {

/* cell (i, k): 8 + 8 (+ 4) bytes, column-major */
static __device__ __forceinline__ void cl_store(const CLParams &A, uint64_t i, uint32_t k, const CLCell &c)
{
    const uint64_t at = (uint64_t)k * A.n + i;
    A.val[at] = c.val;
    A.cell[at] = cl_cell_word(c);
    if (A.len) A.len[at] = c.len;
}

/* Pair q = (message q / P, column q % P) of the pair pass (walk_kern.h): the P
 * pairs of a message in neighbouring lanes, tget's geometry at its spacing 1 */
struct ColsOp {
    using Params = CLParams;
    using Lds = TGLdsFrames;
    using Deep = TGDeepFrames;
    static __device__ __forceinline__ uint64_t pairs(const CLParams &A) { return A.tg.pairs; }
    static __device__ __forceinline__ WalkQueue queue(const CLParams &A) { return walk_queue(A.tg); }
    template <class FR>
    static __device__ __forceinline__ bool pair(const CLParams &A, uint64_t q, const FR &fr, bool last)
    {
        const uint64_t i = q / A.tg.P;
        const uint32_t k = (uint32_t)(q - i * A.tg.P);
        const uint64_t a = A.tg.in_off[i], e = A.tg.in_off[i + 1];
        TGRes r = tg_walk(A.tg, A.tg.src + a, e - a, k, fr);
        if (r.status == TG_ST_DEEP) {
            if (!last) return true;
            r = tg_res(DG_TGET_E_READ, r.step); /* unreachable: 1023 levels fit */
        }
        cl_store(A, i, k, cl_cell((uint32_t)(A.kinds >> (k * 8)) & 0xFFu, r, A.tg.src + a, a));
        return false;
    }
    template <class FR>
    static __device__ __forceinline__ bool lane(const CLParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, false); }
    template <class FR>
    static __device__ __forceinline__ bool deep(const CLParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, true); }
};

/* The emit: a block takes a chunk of CL_EMIT_CHUNK neighbouring elements a
 * round; in step r lane t takes element g = base + r * CL_BLOCK + t and stores
 * elems[g], so every wave store is 512 contiguous bytes. A lane finds its
 * message by a binary search in elem_off. NARROW: the block's first and last
 * lane search all n messages for the chunk's first and last element, and every
 * element is then searched only between their two answers, which is where the
 * chunk's elements lie (a step or two when lists are long): two searches of
 * full depth, each a chain of dependent loads, per chunk instead of per
 * element. No element at an index >= cap is read or stored. */
template <bool NARROW>
__global__ __launch_bounds__(CL_BLOCK) void cols_emit_kernel(CLEmit E)
{
    __shared__ uint64_t range[2];
    const uint64_t need = E.elem_off[E.n], total = need < E.cap ? need : E.cap;
    for (uint64_t base = (uint64_t)blockIdx.x * CL_EMIT_CHUNK; base < total; base += (uint64_t)gridDim.x * CL_EMIT_CHUNK) {
        const uint64_t end = base + CL_EMIT_CHUNK < total ? base + CL_EMIT_CHUNK : total;
        uint64_t lo = 0, hi = E.n;
        if (NARROW) {
            if (threadIdx.x == 0) range[0] = cl_find(E.elem_off, 0, E.n, base);
            if (threadIdx.x == CL_BLOCK - 1) range[1] = cl_find(E.elem_off, 0, E.n, end - 1);
            __syncthreads();
            lo = range[0], hi = range[1] + 1;
            __syncthreads(); /* the next round writes range again */
        }
        for (uint64_t g = base + threadIdx.x; g < end; g += CL_BLOCK) {
            const uint64_t m = cl_find(E.elem_off, lo, hi, g);
            const uint32_t et = (uint32_t)(E.cell[m] >> 8) & 0xFFu;
            E.elems[g] = cl_elem(E.src, E.val[m], et, g - E.elem_off[m]);
        }
    }
}

void launch_cols_pass(hipStream_t s, const CLParams &A) { launch_walk<ColsOp>(s, A, A.tg.pairs); }

void launch_cols_scan(hipStream_t s, const uint32_t *cnt, uint64_t n, uint64_t *sums, uint64_t *off)
{
    launch_scan(s, ScanU32{cnt}, n, sums, off);
}

void launch_cols_emit(hipStream_t s, const CLEmit &E, uint32_t max_blocks, bool full_search)
{
    const uint64_t chunks = (E.cap + CL_EMIT_CHUNK - 1) / CL_EMIT_CHUNK; /* no more elements than cap are stored */
    const uint32_t blocks = (uint32_t)(chunks < max_blocks ? chunks : max_blocks);
    if (full_search) hipLaunchKernelGGL(cols_emit_kernel<false>, dim3(blocks), dim3(CL_BLOCK), 0, s, E);
    else hipLaunchKernelGGL(cols_emit_kernel<true>, dim3(blocks), dim3(CL_BLOCK), 0, s, E);
}

}  // namespace dg
