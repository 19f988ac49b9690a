/* vals kernels (typed column writes, vals_device.h): the size pass, the
 * offsets' shift to out_base, the head pass (with LANE the cell's whole body
 * too) and the wave-parallel body pass. The scan between them is cols'. */
#include "vals_device.h"

namespace dg {

/* One lane per cell, the K cells of a message in neighbouring lanes. CLOSED (a
 * plan of scalars, every field present): the offsets are base + i * msg +
 * pre[j], written here with the bytes; otherwise the lengths go to the scan. */
template <bool CLOSED>
__global__ __launch_bounds__(VL_BLOCK) void vals_size_kernel(VLParams A)
{
    const uint64_t q = (uint64_t)blockIdx.x * VL_BLOCK + threadIdx.x;
    if (q >= A.pairs) return;
    const VLPair p = vl_pair(A, q);
    if (A.status) A.status[q] = (uint8_t)p.z.status;
    if (!CLOSED) {
        A.len[q] = p.z.len;
        return;
    }
    const uint64_t pos = A.base + (uint64_t)p.i * A.msg + A.pre[p.j];
    A.off[q] = pos;
    if (q == A.pairs - 1) A.off[A.pairs] = pos + p.z.len;
    if (A.out) vl_head(p.kind, p.id, p.fh, p.stop, p.z, p.v, A.out, pos, A.cap);
}

/* the scan starts at 0: every offset moves to out_base */
__global__ __launch_bounds__(VL_BLOCK) void vals_rebase_kernel(uint64_t *off, uint64_t entries, uint64_t base)
{
    const uint64_t q = (uint64_t)blockIdx.x * VL_BLOCK + threadIdx.x;
    if (q < entries) off[q] += base;
}

/* One lane per cell: what precedes the body, and STOP. LANE: the body too,
 * unit after unit (the baseline). */
template <bool LANE>
__global__ __launch_bounds__(VL_BLOCK) void vals_head_kernel(VLParams A)
{
    const uint64_t q = (uint64_t)blockIdx.x * VL_BLOCK + threadIdx.x;
    if (q >= A.pairs) return;
    const VLPair p = vl_pair(A, q);
    const uint64_t pos = A.off[q];
    vl_head(p.kind, p.id, p.fh, p.stop, p.z, p.v, A.out, pos, A.cap);
    if (LANE) vl_body_loop(A, p, pos);
}

/* The body pass, in cols_emit_kernel's geometry over the arena's bytes: a
 * block takes VL_CHUNK neighbouring bytes a round, its first and last lane
 * search all cells for the chunk's first and last byte, and in step r lane t
 * takes the 8 bytes at base + (r * VL_BLOCK + t) * 8 (vl_granule). */
__global__ __launch_bounds__(VL_BLOCK) void vals_body_kernel(VLParams A)
{
    __shared__ uint64_t range[2];
    const uint64_t need = A.off[A.pairs], total = need < A.cap ? need : A.cap;
    const uint64_t first = A.base & ~(uint64_t)(VL_UNIT - 1);
    for (uint64_t base = first + (uint64_t)blockIdx.x * VL_CHUNK; base < total; base += (uint64_t)gridDim.x * VL_CHUNK) {
        const uint64_t end = base + VL_CHUNK < total ? base + VL_CHUNK : total;
        if (threadIdx.x == 0) range[0] = cl_find(A.off, 0, A.pairs, base > A.base ? base : A.base);
        if (threadIdx.x == VL_BLOCK - 1) range[1] = cl_find(A.off, 0, A.pairs, end - 1);
        __syncthreads();
        const uint64_t lo = range[0], hi = range[1] + 1;
        __syncthreads(); /* the next round writes range again */
        for (uint64_t p = base + (uint64_t)threadIdx.x * VL_UNIT; p < end; p += (uint64_t)VL_BLOCK * VL_UNIT)
            vl_granule(A, lo, hi, p, total);
    }
}

void launch_vals_size(hipStream_t s, const VLParams &A, bool closed)
{
    if (closed) hipLaunchKernelGGL(vals_size_kernel<true>, cell_grid(A.pairs), dim3(VL_BLOCK), 0, s, A);
    else hipLaunchKernelGGL(vals_size_kernel<false>, cell_grid(A.pairs), dim3(VL_BLOCK), 0, s, A);
}

void launch_vals_rebase(hipStream_t s, uint64_t *off, uint64_t entries, uint64_t base)
{
    hipLaunchKernelGGL(vals_rebase_kernel, cell_grid(entries), dim3(VL_BLOCK), 0, s, off, entries, base);
}

void launch_vals_emit(hipStream_t s, const VLParams &A, uint32_t max_blocks, bool lane_emit, bool bodies)
{
    if (lane_emit) {
        hipLaunchKernelGGL(vals_head_kernel<true>, cell_grid(A.pairs), dim3(VL_BLOCK), 0, s, A);
        return;
    }
    hipLaunchKernelGGL(vals_head_kernel<false>, cell_grid(A.pairs), dim3(VL_BLOCK), 0, s, A);
    if (!bodies) return; /* a plan of scalars */
    /* no byte at cap or beyond is stored, so no more chunks than lie below cap */
    const uint64_t first = A.base & ~(uint64_t)(VL_UNIT - 1);
    const uint64_t chunks = (A.cap - first + VL_CHUNK - 1) / VL_CHUNK;
    const uint32_t blocks = (uint32_t)(chunks < max_blocks ? chunks : max_blocks);
    hipLaunchKernelGGL(vals_body_kernel, dim3(blocks), dim3(VL_BLOCK), 0, s, A);
}

}  // namespace dg
