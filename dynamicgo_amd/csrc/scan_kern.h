/*
 * scan_kern.h — the one scan of counts into 64-bit offsets: off[i] = the sum
 * of count(0..i), off[n] the total. Three small kernels over tiles of SCAN_TILE
 * counts: tile sums, their exclusive scan by one block, then every tile's own
 * scan on top of its base. Any n below 2^32: the tile sums are scanned in a
 * loop with a carry. CNT says how count i is read: a dg_kids_head's field
 * (kids) or a plain u32 (cols, and through launch_cols_scan ents, rows, vals
 * and evals). Included by kids_kern.hip and cols_kern.hip only.
 */
#pragma once
#include "scan_defs.h"
#include "tget_device.h"

namespace dg {

static_assert(SCAN_TILE % SCAN_BLOCK == 0, "whole counts per lane");

struct ScanU32 {
    const uint32_t *cnt;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return cnt[i]; }
};
struct ScanKidsHead {
    const dg_kids_head *head;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return head[i].count; }
};

static __device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t *sh, uint64_t &total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < SCAN_BLOCK; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    total = sh[SCAN_BLOCK - 1];
    __syncthreads();
    return incl - v; /* exclusive */
}

template <class CNT>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_sums_kernel(CNT cnt, uint64_t n, uint64_t *sums)
{
    __shared__ uint64_t sh[SCAN_BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    uint64_t v = 0;
    for (uint32_t j = 0; j < SCAN_TILE / SCAN_BLOCK; j++) {
        const uint64_t i = base + j * SCAN_BLOCK + threadIdx.x;
        if (i < n) v += cnt(i);
    }
    uint64_t total;
    (void)block_scan(v, sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

/* reads no count: a template so that each unit that launches it has its own */
template <class CNT>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_bases_kernel(uint64_t *sums, uint64_t tiles)
{
    __shared__ uint64_t sh[SCAN_BLOCK];
    uint64_t carry = 0;
    for (uint64_t q = 0; q < tiles; q += SCAN_BLOCK) {
        const uint64_t i = q + threadIdx.x;
        const uint64_t v = i < tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_scan(v, sh, total);
        if (i < tiles) sums[i] = carry + ex;
        carry += total;
    }
}

/* sums = the tiles' bases, or null for a batch of one tile */
template <class CNT>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_tile_kernel(CNT cnt, uint64_t n, const uint64_t *sums, uint64_t *off)
{
    __shared__ uint64_t sh[SCAN_BLOCK];
    constexpr uint32_t PER = SCAN_TILE / SCAN_BLOCK;
    const uint64_t first = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * PER;
    uint32_t c[PER];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        c[j] = first + j < n ? cnt(first + j) : 0u;
        v += c[j];
    }
    uint64_t total;
    uint64_t o = block_scan(v, sh, total) + (sums ? sums[blockIdx.x] : 0ull);
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        if (first + j >= n) continue;
        off[first + j] = o;
        o += c[j];
        if (first + j == n - 1) off[n] = o;
    }
}

/* sums: room for a u64 per tile (unused for a batch of one tile) */
template <class CNT>
static inline void launch_scan(hipStream_t s, CNT cnt, uint64_t n, uint64_t *sums, uint64_t *off)
{
    const uint32_t tiles = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
    if (tiles > 1) {
        hipLaunchKernelGGL(scan_sums_kernel<CNT>, dim3(tiles), dim3(SCAN_BLOCK), 0, s, cnt, n, sums);
        hipLaunchKernelGGL(scan_bases_kernel<CNT>, dim3(1), dim3(SCAN_BLOCK), 0, s, sums, (uint64_t)tiles);
    }
    hipLaunchKernelGGL(scan_tile_kernel<CNT>, dim3(tiles), dim3(SCAN_BLOCK), 0, s, cnt, n, tiles > 1 ? sums : nullptr, off);
}

}  // namespace dg
