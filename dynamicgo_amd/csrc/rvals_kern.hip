/* rvals kernels (row column writes, rvals_device.h): the cell-size pass, the
 * message pass, the head pass and the wave-parallel body pass. The scans
 * between them are cols' (cols_kern.hip), the offsets' shift to out_base vals'. */
#include "rvals_device.h"

namespace dg {

/* One lane per cell, the K cells of a row in neighbouring lanes: the item's
 * length for the scan and the cell status. */
__global__ __launch_bounds__(RV_BLOCK) void rvals_size_kernel(RVParams A)
{
    const uint64_t q = (uint64_t)blockIdx.x * RV_BLOCK + threadIdx.x;
    if (q < A.cells) rv_size_lane(A, q);
}

/* One lane per message: its status, its length and its rows to emit for the two scans. */
__global__ __launch_bounds__(RV_BLOCK) void rvals_msg_kernel(RVParams A)
{
    const uint64_t i = (uint64_t)blockIdx.x * RV_BLOCK + threadIdx.x;
    if (i < A.n) rv_msg_lane(A, i);
}

/* The head pass. First one lane per message writes the list header (an empty
 * list has one too). Then, in evals_emit_kernel's geometry over the scanned
 * row counts times K: a block takes RV_CHUNK neighbouring emitted cells a round,
 * its first and last lane search all messages for the chunk's first and last
 * row, and in step r lane t takes cell base + r * RV_BLOCK + t and searches
 * between the two answers. */
__global__ __launch_bounds__(RV_BLOCK) void rvals_head_kernel(RVParams A)
{
    __shared__ uint64_t range[2];
    for (uint64_t i = (uint64_t)blockIdx.x * RV_BLOCK + threadIdx.x; i < A.n; i += (uint64_t)gridDim.x * RV_BLOCK)
        rv_list_head(A, i);
    const uint64_t total = A.cnt_off[A.n] * A.K;
    for (uint64_t base = (uint64_t)blockIdx.x * RV_CHUNK; base < total; base += (uint64_t)gridDim.x * RV_CHUNK) {
        const uint64_t end = base + RV_CHUNK < total ? base + RV_CHUNK : total;
        if (threadIdx.x == 0) range[0] = cl_find(A.cnt_off, 0, A.n, base / A.K);
        if (threadIdx.x == RV_BLOCK - 1) range[1] = cl_find(A.cnt_off, 0, A.n, (end - 1) / A.K);
        __syncthreads();
        const uint64_t lo = range[0], hi = range[1] + 1;
        __syncthreads(); /* the next round writes range again */
        for (uint64_t t = base + threadIdx.x; t < end; t += RV_BLOCK) rv_head_lane(A, cl_find(A.cnt_off, lo, hi, t / A.K), t);
    }
}

/* The body pass, in vals_body_kernel's geometry over the arena's bytes: a block
 * takes VL_CHUNK neighbouring bytes a round, its first and last lane search
 * d_out_off for the chunk's first and last byte, and in step r lane t takes the
 * 8 bytes at base + (r * RV_BLOCK + t) * 8 (rv_granule). */
__global__ __launch_bounds__(RV_BLOCK) void rvals_body_kernel(RVParams A)
{
    __shared__ uint64_t range[2];
    const uint64_t need = A.off[A.n], total = need < A.cap ? need : A.cap;
    const uint64_t first = A.base & ~(uint64_t)(VL_UNIT - 1);
    for (uint64_t base = first + (uint64_t)blockIdx.x * VL_CHUNK; base < total; base += (uint64_t)gridDim.x * VL_CHUNK) {
        const uint64_t end = base + VL_CHUNK < total ? base + VL_CHUNK : total;
        if (threadIdx.x == 0) range[0] = cl_find(A.off, 0, A.n, base > A.base ? base : A.base);
        if (threadIdx.x == RV_BLOCK - 1) range[1] = cl_find(A.off, 0, A.n, end - 1);
        __syncthreads();
        const uint64_t lo = range[0], hi = range[1] + 1;
        __syncthreads(); /* the next round writes range again */
        for (uint64_t p = base + (uint64_t)threadIdx.x * VL_UNIT; p < end; p += (uint64_t)RV_BLOCK * VL_UNIT)
            rv_granule(A, lo, hi, p, total);
    }
}

void launch_rvals_size(hipStream_t s, const RVParams &A) { hipLaunchKernelGGL(rvals_size_kernel, cell_grid(A.cells), dim3(RV_BLOCK), 0, s, A); }

void launch_rvals_msgs(hipStream_t s, const RVParams &A) { hipLaunchKernelGGL(rvals_msg_kernel, cell_grid(A.n), dim3(RV_BLOCK), 0, s, A); }

void launch_rvals_emit(hipStream_t s, const RVParams &A, uint32_t head_blocks, uint32_t max_blocks, bool bodies)
{
    hipLaunchKernelGGL(rvals_head_kernel, dim3(head_blocks), dim3(RV_BLOCK), 0, s, A);
    if (!bodies) return; /* a plan of scalars, or no rows */
    /* no byte at cap or beyond is stored, so no more chunks than lie below cap */
    const uint64_t first = A.base & ~(uint64_t)(VL_UNIT - 1);
    const uint64_t chunks = (A.cap - first + VL_CHUNK - 1) / VL_CHUNK;
    const uint32_t blocks = (uint32_t)(chunks < max_blocks ? chunks : max_blocks);
    hipLaunchKernelGGL(rvals_body_kernel, dim3(blocks), dim3(RV_BLOCK), 0, s, A);
}

}  // namespace dg
