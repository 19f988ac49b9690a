/* kids kernels (batched Children, kids_device.h): the count and emit passes with
 * their deep passes, the scan of the counts (scan_kern.h) and the wide emit. */
#include "kids_device.h"
#include "scan_kern.h"

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

void launch_kids_count(hipStream_t s, const KDParams &A)
{
    hipLaunchKernelGGL(kids_kernel<0>, dim3((uint32_t)((A.n + KD_BLOCK - 1) / KD_BLOCK)), dim3(KD_BLOCK), 0, s, A);
    hipLaunchKernelGGL(kids_deep_kernel<0>, dim3(KD_DEEP_BLOCKS), dim3(KD_DEEP_BLOCK), 0, s, A);
}

/* rec_off[i] = the sum of head[0..i).count as 64-bit, rec_off[n] the total */
void launch_kids_scan(hipStream_t s, const KDParams &A, uint64_t *sums)
{
    launch_scan(s, ScanKidsHead{A.head}, A.n, sums, A.rec_off);
}

void launch_kids_emit(hipStream_t s, const KDParams &A, uint32_t wide_blocks)
{
    hipLaunchKernelGGL(kids_kernel<1>, dim3((uint32_t)((A.n + KD_BLOCK - 1) / KD_BLOCK)), dim3(KD_BLOCK), 0, s, A);
    hipLaunchKernelGGL(kids_deep_kernel<1>, dim3(KD_DEEP_BLOCKS), dim3(KD_DEEP_BLOCK), 0, s, A);
    if (A.wide_min) hipLaunchKernelGGL(kids_wide_kernel, dim3(wide_blocks), dim3(KD_WIDE_BLOCK), 0, s, A);
}

}  // namespace dg
