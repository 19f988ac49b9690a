/* kids kernels (batched Children, kids_device.h): the count and emit passes with
 * their deep passes, the scan of the counts and the wide emit. */
#include "kids_device.h"

namespace dg {

/* the emit pass's gate for message i: false = nothing to emit (no records, a
 * failed message, or records that would pass rec_cap: DG_KIDS_E_OVERFLOW, set
 * here). A head left DG_KIDS_E_OVERFLOW by an earlier call is judged again. */
static __device__ __forceinline__ bool kd_emit_gate(const KDParams &A, uint64_t i, uint32_t &cnt, dg_kids_head &h)
{
    h = A.head[i];
    if (h.status != DG_TGET_OK && h.status != DG_KIDS_E_OVERFLOW) return false;
    const uint64_t off = A.rec_off[i], c = A.rec_off[i + 1] - off;
    cnt = (uint32_t)c;
    if (!c) return false;
    if (off + c > A.rec_cap) {
        if (h.status == DG_TGET_OK) kd_put_head(A.head + i, 0, h.direct, h.start, h.type, h.key_type, h.elem_type, DG_KIDS_E_OVERFLOW);
        return false;
    }
    if (h.status != DG_TGET_OK) kd_put_head(A.head + i, cnt, h.direct, h.start, h.type, h.key_type, h.elem_type, DG_TGET_OK);
    return true;
}

/* One lane per message. EMIT 0: the count pass (kd_count_msg). EMIT 1: the emit
 * pass; a node the wide kernel takes is queued for it. Messages nested beyond
 * the LDS levels are queued for kids_deep_kernel. */
template <int EMIT>
__global__ __launch_bounds__(KD_BLOCK) void kids_kernel(KDParams A)
{
    __shared__ uint64_t lf[2 * KD_LDS_DEPTH * KD_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * KD_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const KDLdsFrames fr{&lf[threadIdx.x]};
    bool deep;
    if (!EMIT) {
        deep = kd_count_msg(A, i, fr);
    } else {
        uint32_t cnt;
        dg_kids_head h;
        if (!kd_emit_gate(A, i, cnt, h)) return;
        if (A.wide_min && h.direct >= A.wide_min && kd_wide_ok(h)) {
            A.wide_list[atomicAdd(A.cnt + 1, 1u)] = (uint32_t)i;
            return;
        }
        deep = kd_emit_msg(A, i, cnt, fr);
    }
    if (deep) A.deep_list[atomicAdd(A.cnt, 1u)] = (uint32_t)i;
}

/* the queued messages again from the start with KD_DEEP_DEPTH levels per lane
 * in device memory; a small grid striding over the queue. Also zeroes the
 * counters the previous stage used. */
template <int EMIT>
__global__ __launch_bounds__(KD_DEEP_BLOCK) void kids_deep_kernel(KDParams A)
{
    const uint32_t cnt = *(volatile const uint32_t *)A.cnt;
    const uint32_t lane = blockIdx.x * KD_DEEP_BLOCK + threadIdx.x;
    if (lane == 0) {
        A.reset[0] = 0, A.reset[1] = 0;
        if (cnt) atomicAdd(A.stats + KD_STAT_DEEP, (unsigned long long)cnt);
    }
    const KDDeepFrames fr{A.ws + lane};
    for (uint32_t g = lane; g < cnt; g += KD_DEEP_LANES) {
        const uint64_t i = A.deep_list[g];
        if (!EMIT) {
            if (kd_count_msg(A, i, fr)) /* unreachable: 1023 levels fit */
                kd_put_head(A.head + i, 0, A.n_steps, 0, 0, 0, 0, DG_TGET_E_READ);
        } else {
            (void)kd_emit_msg(A, i, (uint32_t)(A.rec_off[i + 1] - A.rec_off[i]), fr);
        }
    }
}

/* The wide route: a queued node's children sit at start + header + j * size,
 * so one lane makes one record from j alone (plus the load of an int key) and
 * a wave stores 64 neighbouring records. The count pass has checked that all
 * of them lie inside the message. */
__global__ __launch_bounds__(KD_WIDE_BLOCK) void kids_wide_kernel(KDParams A)
{
    const uint32_t cnt = *(volatile const uint32_t *)(A.cnt + 1);
    for (uint32_t g = blockIdx.x; g < cnt; g += gridDim.x) {
        const uint64_t i = A.wide_list[g];
        const dg_kids_head h = A.head[i];
        const uint64_t a = A.tg.in_off[i], len = A.tg.in_off[i + 1] - a;
        const uint8_t *b = A.tg.src + a;
        dg_kid_rec *out = A.recs + A.rec_off[i];
        const uint32_t count = (uint32_t)(A.rec_off[i + 1] - A.rec_off[i]); /* what the gate found to fit */
        const bool map = h.type == TT_MAP;
        const uint32_t kt = h.key_type, ks = map ? tg_fixed(kt) : 0u, vs = tg_fixed(h.elem_type);
        const bool intkey = kt == TT_BYTE || kt == TT_I16 || kt == TT_I32 || kt == TT_I64;
        const uint64_t first = (uint64_t)h.start + (map ? 6 : 5);
        for (uint32_t j = threadIdx.x; j < count; j += KD_WIDE_BLOCK) {
            const uint64_t ent = first + (uint64_t)j * (ks + vs), start = ent + ks;
            if (start + vs > len) break; /* heads of another batch (a wrong DG_KIDS_F_COUNTED call): read nothing outside */
            int64_t key = j;
            uint32_t kind = DG_PS_INDEX;
            if (map && intkey) {
                const uint64_t raw = __builtin_bswap64(tg_ld(b + ent).lo);
                key = kt == TT_BYTE ? (int64_t)(raw >> 56) : (int64_t)raw >> (64 - 8 * ks);
                kind = DG_PS_INTKEY;
            } else if (map) {
                key = ks, kind = DG_PS_BINKEY;
            }
            uint4 lo, hi;
            lo.x = (uint32_t)start, lo.y = (uint32_t)(start + vs), lo.z = (uint32_t)ent, lo.w = DG_KIDS_NO_PARENT;
            hi.x = (uint32_t)(uint64_t)key, hi.y = (uint32_t)((uint64_t)key >> 32);
            hi.z = (uint32_t)h.elem_type | kind << 8 | 1u << 16, hi.w = 0;
            uint4 *r = (uint4 *)(void *)(out + j);
            r[0] = lo, r[1] = hi;
        }
    }
}

/* ---- the scan: rec_off[i] = the sum of head[0..i).count as 64-bit, rec_off[n]
 * the total. Three small kernels over tiles of KD_SCAN_TILE counts: tile sums,
 * their exclusive scan by one block, then every tile's own scan on top of its
 * base. Any n below 2^32: the tile sums are scanned in a loop with a carry. */
static __device__ __forceinline__ uint64_t kd_block_scan(uint64_t v, uint64_t *sh, uint64_t &total)
{
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < KD_BLOCK; d <<= 1) {
        const uint64_t x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    total = sh[KD_BLOCK - 1];
    __syncthreads();
    return incl - v; /* exclusive */
}

__global__ __launch_bounds__(KD_BLOCK) void kids_scan_sums_kernel(const dg_kids_head *head, uint64_t n, uint64_t *sums)
{
    __shared__ uint64_t sh[KD_BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * KD_SCAN_TILE;
    uint64_t v = 0;
    for (uint32_t j = 0; j < KD_SCAN_TILE / KD_BLOCK; j++) {
        const uint64_t i = base + j * KD_BLOCK + threadIdx.x;
        if (i < n) v += head[i].count;
    }
    uint64_t total;
    (void)kd_block_scan(v, sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(KD_BLOCK) void kids_scan_bases_kernel(uint64_t *sums, uint64_t tiles)
{
    __shared__ uint64_t sh[KD_BLOCK];
    uint64_t carry = 0;
    for (uint64_t q = 0; q < tiles; q += KD_BLOCK) {
        const uint64_t i = q + threadIdx.x;
        const uint64_t v = i < tiles ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = kd_block_scan(v, sh, total);
        if (i < tiles) sums[i] = carry + ex;
        carry += total;
    }
}

/* sums = the tiles' bases, or null for a batch of one tile */
__global__ __launch_bounds__(KD_BLOCK) void kids_scan_tile_kernel(const dg_kids_head *head, uint64_t n, const uint64_t *sums,
                                                                  uint64_t *rec_off)
{
    __shared__ uint64_t sh[KD_BLOCK];
    constexpr uint32_t PER = KD_SCAN_TILE / KD_BLOCK;
    const uint64_t first = (uint64_t)blockIdx.x * KD_SCAN_TILE + (uint64_t)threadIdx.x * PER;
    uint32_t c[PER];
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        c[j] = first + j < n ? head[first + j].count : 0u;
        v += c[j];
    }
    uint64_t total;
    uint64_t off = kd_block_scan(v, sh, total) + (sums ? sums[blockIdx.x] : 0ull);
#pragma unroll
    for (uint32_t j = 0; j < PER; j++) {
        if (first + j >= n) continue;
        rec_off[first + j] = off;
        off += c[j];
        if (first + j == n - 1) rec_off[n] = off;
    }
}

void launch_kids_count(hipStream_t s, const KDParams &A)
{
    hipLaunchKernelGGL(kids_kernel<0>, dim3((uint32_t)((A.n + KD_BLOCK - 1) / KD_BLOCK)), dim3(KD_BLOCK), 0, s, A);
    hipLaunchKernelGGL(kids_deep_kernel<0>, dim3(KD_DEEP_BLOCKS), dim3(KD_DEEP_BLOCK), 0, s, A);
}

void launch_kids_scan(hipStream_t s, const KDParams &A, uint64_t *sums)
{
    const uint32_t tiles = (uint32_t)((A.n + KD_SCAN_TILE - 1) / KD_SCAN_TILE);
    if (tiles > 1) {
        hipLaunchKernelGGL(kids_scan_sums_kernel, dim3(tiles), dim3(KD_BLOCK), 0, s, A.head, A.n, sums);
        hipLaunchKernelGGL(kids_scan_bases_kernel, dim3(1), dim3(KD_BLOCK), 0, s, sums, (uint64_t)tiles);
    }
    hipLaunchKernelGGL(kids_scan_tile_kernel, dim3(tiles), dim3(KD_BLOCK), 0, s, A.head, A.n, tiles > 1 ? sums : nullptr,
                       A.rec_off);
}

void launch_kids_emit(hipStream_t s, const KDParams &A, uint32_t wide_blocks)
{
    hipLaunchKernelGGL(kids_kernel<1>, dim3((uint32_t)((A.n + KD_BLOCK - 1) / KD_BLOCK)), dim3(KD_BLOCK), 0, s, A);
    hipLaunchKernelGGL(kids_deep_kernel<1>, dim3(KD_DEEP_BLOCKS), dim3(KD_DEEP_BLOCK), 0, s, A);
    if (A.wide_min) hipLaunchKernelGGL(kids_wide_kernel, dim3(wide_blocks), dim3(KD_WIDE_BLOCK), 0, s, A);
}

}  // namespace dg
