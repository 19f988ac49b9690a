/* cols kernels (typed column reads, cols_device.h): the cell pass with its deep
 * pass, the scan of a list column's counts and the element-parallel emit. */
#include "cols_device.h"

namespace dg {

/* cell (i, k): 8 + 8 (+ 4) bytes, column-major */
static __device__ __forceinline__ void cl_store(const CLParams &A, uint64_t i, uint32_t k, const CLCell &c)
{
    const uint64_t at = (uint64_t)k * A.n + i;
    A.val[at] = c.val;
    A.cell[at] = cl_cell_word(c);
    if (A.len) A.len[at] = c.len;
}

/* One lane per (message, column) pair, the P pairs of a message in
 * neighbouring lanes (tget_kernel's geometry at its spacing 1). Pairs whose
 * skip nests beyond the LDS frames are queued for cols_deep_kernel. */
__global__ __launch_bounds__(TG_BLOCK) void cols_kernel(CLParams A)
{
    __shared__ uint64_t lf[TG_LDS_DEPTH * TG_BLOCK];
    const uint64_t q = (uint64_t)blockIdx.x * TG_BLOCK + threadIdx.x;
    if (q >= A.tg.pairs) return;
    const uint64_t i = q / A.tg.P;
    const uint32_t k = (uint32_t)(q - i * A.tg.P);
    const uint64_t a = A.tg.in_off[i], e = A.tg.in_off[i + 1];
    const TGLdsFrames fr{&lf[threadIdx.x]};
    const TGRes r = tg_walk(A.tg, A.tg.src + a, e - a, k, fr);
    if (r.status == TG_ST_DEEP) {
        A.tg.deep_list[atomicAdd(A.tg.deep_count, 1u)] = (uint32_t)q;
        return;
    }
    cl_store(A, i, k, cl_cell((uint32_t)(A.kinds >> (k * 8)) & 0xFFu, r, A.tg.src + a, a));
}

/* the queued pairs again with TG_DEEP_DEPTH frames per lane in device memory;
 * also zeroes the counter the previous launch used */
__global__ __launch_bounds__(TG_DEEP_BLOCK) void cols_deep_kernel(CLParams A)
{
    const uint32_t cnt = *(volatile const uint32_t *)A.tg.deep_count;
    const uint32_t lane = blockIdx.x * TG_DEEP_BLOCK + threadIdx.x;
    if (lane == 0) *A.tg.reset_count = 0;
    const TGDeepFrames fr{A.tg.ws + lane};
    for (uint32_t g = lane; g < cnt; g += TG_DEEP_LANES) {
        const uint64_t q = A.tg.deep_list[g];
        const uint64_t i = q / A.tg.P;
        const uint32_t k = (uint32_t)(q - i * A.tg.P);
        const uint64_t a = A.tg.in_off[i], e = A.tg.in_off[i + 1];
        TGRes r = tg_walk(A.tg, A.tg.src + a, e - a, k, fr);
        if (r.status == TG_ST_DEEP) r = tg_res(DG_TGET_E_READ, r.step); /* unreachable: 1023 levels fit */
        cl_store(A, i, k, cl_cell((uint32_t)(A.kinds >> (k * 8)) & 0xFFu, r, A.tg.src + a, a));
    }
}

/* ---- the scan: off[i] = the sum of cnt[0..i) as 64-bit, off[n] the total.
 * The kids scan (kids_kern.hip) restated over plain u32 counts: tile sums, their
 * exclusive scan by one block with a carry, then every tile's own scan on top
 * of its base. */
static __device__ __forceinline__ uint64_t cl_block_scan(uint64_t v, uint64_t *sh, uint64_t &total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < CL_BLOCK; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    total = sh[CL_BLOCK - 1];
    __syncthreads();
    return incl - v; /* exclusive */
}

__global__ __launch_bounds__(CL_BLOCK) void cols_scan_sums_kernel(const uint32_t *cnt, uint64_t n, uint64_t *sums)
{
    __shared__ uint64_t sh[CL_BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * CL_SCAN_TILE;
    uint64_t v = 0;
    for (uint32_t j = 0; j < CL_SCAN_TILE / CL_BLOCK; j++) {
        const uint64_t i = base + j * CL_BLOCK + threadIdx.x;
        if (i < n) v += cnt[i];
    }
    uint64_t total;
    (void)cl_block_scan(v, sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(CL_BLOCK) void cols_scan_bases_kernel(uint64_t *sums, uint64_t tiles)
{
    __shared__ uint64_t sh[CL_BLOCK];
    uint64_t carry = 0;
    for (uint64_t q = 0; q < tiles; q += CL_BLOCK) {
        const uint64_t i = q + threadIdx.x;
        const uint64_t v = i < tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = cl_block_scan(v, sh, total);
        if (i < tiles) sums[i] = carry + ex;
        carry += total;
    }
}

/* sums = the tiles' bases, or null for a batch of one tile */
__global__ __launch_bounds__(CL_BLOCK) void cols_scan_tile_kernel(const uint32_t *cnt, uint64_t n, const uint64_t *sums,
                                                                  uint64_t *off)
{
    __shared__ uint64_t sh[CL_BLOCK];
    constexpr uint32_t PER = CL_SCAN_TILE / CL_BLOCK;
    const uint64_t first = (uint64_t)blockIdx.x * CL_SCAN_TILE + (uint64_t)threadIdx.x * PER;
    uint32_t c[PER];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        c[j] = first + j < n ? cnt[first + j] : 0u;
        v += c[j];
    }
    uint64_t total;
    uint64_t o = cl_block_scan(v, sh, total) + (sums ? sums[blockIdx.x] : 0ull);
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        if (first + j >= n) continue;
        off[first + j] = o;
        o += c[j];
        if (first + j == n - 1) off[n] = o;
    }
}

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

void launch_cols_pass(hipStream_t s, const CLParams &A)
{
    const dim3 grid((uint32_t)((A.tg.pairs + TG_BLOCK - 1) / TG_BLOCK)), block(TG_BLOCK);
    hipLaunchKernelGGL(cols_kernel, grid, block, 0, s, A);
    hipLaunchKernelGGL(cols_deep_kernel, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

void launch_cols_scan(hipStream_t s, const uint32_t *cnt, uint64_t n, uint64_t *sums, uint64_t *off)
{
    const uint32_t tiles = (uint32_t)((n + CL_SCAN_TILE - 1) / CL_SCAN_TILE);
    if (tiles > 1) {
        hipLaunchKernelGGL(cols_scan_sums_kernel, dim3(tiles), dim3(CL_BLOCK), 0, s, cnt, n, sums);
        hipLaunchKernelGGL(cols_scan_bases_kernel, dim3(1), dim3(CL_BLOCK), 0, s, sums, (uint64_t)tiles);
    }
    hipLaunchKernelGGL(cols_scan_tile_kernel, dim3(tiles), dim3(CL_BLOCK), 0, s, cnt, n, tiles > 1 ? sums : nullptr, off);
}

void launch_cols_emit(hipStream_t s, const CLEmit &E, uint32_t max_blocks, bool full_search)
{
    const uint64_t chunks = (E.cap + CL_EMIT_CHUNK - 1) / CL_EMIT_CHUNK; /* no more elements than cap are stored */
    const uint32_t blocks = (uint32_t)(chunks < max_blocks ? chunks : max_blocks);
    if (full_search) hipLaunchKernelGGL(cols_emit_kernel<false>, dim3(blocks), dim3(CL_BLOCK), 0, s, E);
    else hipLaunchKernelGGL(cols_emit_kernel<true>, dim3(blocks), dim3(CL_BLOCK), 0, s, E);
}

}  // namespace dg
