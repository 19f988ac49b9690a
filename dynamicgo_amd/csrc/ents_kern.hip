/* ents kernels (entry columns, ents_device.h): the cell pass (walk_kern.h),
 * the fixed-stride emit and the two shapes of the variable-stride emit. The
 * scan of the counts is cols' (launch_cols_scan). */
#include "ents_device.h"
#include "walk_kern.h"

namespace dg {

/* cell (i, k): 8 + 8 + 4 + 4 bytes, column-major */
static __device__ __forceinline__ void en_store(const ENParams &A, uint64_t i, uint32_t k, const ENCell &c)
{
    const uint64_t at = (uint64_t)k * A.n + i;
    A.val[at] = c.c.val;
    A.cell[at] = cl_cell_word(c.c);
    A.len[at] = c.c.len;
    A.span[at] = c.span;
}

/* Pair q = (message q / P, column q % P) of the pair pass (walk_kern.h), as cols' */
struct EntsOp {
    using Params = ENParams;
    using Lds = TGLdsFrames;
    using Deep = TGDeepFrames;
    static __device__ __forceinline__ uint64_t pairs(const ENParams &A) { return A.tg.pairs; }
    static __device__ __forceinline__ WalkQueue queue(const ENParams &A) { return walk_queue(A.tg); }
    template <class FR>
    static __device__ __forceinline__ bool pair(const ENParams &A, uint64_t q, const FR &fr, bool last)
    {
        const uint64_t i = q / A.tg.P;
        const uint32_t k = (uint32_t)(q - i * A.tg.P);
        const uint64_t a = A.tg.in_off[i], e = A.tg.in_off[i + 1];
        TGRes r = tg_walk(A.tg, A.tg.src + a, e - a, k, fr);
        if (r.status == TG_ST_DEEP) {
            if (!last) return true;
            r = tg_res(DG_TGET_E_READ, r.step); /* unreachable: 1023 levels fit */
        }
        en_store(A, i, k, en_cell((uint32_t)(A.kinds >> (k * 8)) & 0xFFu, r, A.tg.src + a, a));
        return false;
    }
    template <class FR>
    static __device__ __forceinline__ bool lane(const ENParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, false); }
    template <class FR>
    static __device__ __forceinline__ bool deep(const ENParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, true); }
};

/* The fixed-stride emit, in the shape of cols_emit_kernel: a block takes a
 * chunk of EN_EMIT_CHUNK neighbouring entries a round; its first and last lane
 * search all n messages for the chunk's two ends, and every entry is searched
 * between their answers. Lane t stores key[g] and v[g] of entry g = base + r *
 * EN_BLOCK + t: every wave store is 512 contiguous bytes in each array. No
 * entry at an index >= cap is read or stored, and none that would pass its
 * cell's span. */
__global__ __launch_bounds__(EN_BLOCK) void ents_emit_fixed_kernel(ENEmit E)
{
    __shared__ uint64_t range[2];
    const uint64_t need = E.off[E.n], total = need < E.cap ? need : E.cap;
    const uint32_t v = E.kind & 15u;
    for (uint64_t base = (uint64_t)blockIdx.x * EN_EMIT_CHUNK; base < total; base += (uint64_t)gridDim.x * EN_EMIT_CHUNK) {
        const uint64_t end = base + EN_EMIT_CHUNK < total ? base + EN_EMIT_CHUNK : total;
        if (threadIdx.x == 0) range[0] = cl_find(E.off, 0, E.n, base);
        if (threadIdx.x == EN_BLOCK - 1) range[1] = cl_find(E.off, 0, E.n, end - 1);
        __syncthreads();
        const uint64_t lo = range[0], hi = range[1] + 1;
        __syncthreads(); /* the next round writes range again */
        for (uint64_t g = base + threadIdx.x; g < end; g += EN_BLOCK) {
            const uint64_t m = cl_find(E.off, lo, hi, g);
            const uint32_t aux = (uint32_t)(E.cell[m] >> 32), kt = aux & 0xFFu, vt = aux >> 8 & 0xFFu;
            const uint64_t j = g - E.off[m];
            if ((j + 1) * (tg_fixed(kt) + tg_fixed(vt)) > E.span[m]) continue;
            const ENEntry en = en_fixed(E.src, E.val[m], v, kt, vt, j);
            if (E.key) E.key[g] = en.key;
            if (E.v) E.v[g] = en.val;
        }
    }
}

static __device__ __forceinline__ void en_put(const ENEmit &E, uint64_t o, const ENEntry &en)
{
    if (E.key) E.key[o] = en.key;
    if (E.klen) E.klen[o] = en.klen;
    if (E.v) E.v[o] = en.val;
    if (E.vlen) E.vlen[o] = en.vlen;
}

/* what a lane of the variable-stride emit walks: message i's cell when it is
 * OK and not empty (left = 0 otherwise) */
struct ENWalk {
    uint64_t p, e, o;
    uint32_t left, kt, vt;
};
static __device__ __forceinline__ ENWalk en_walk_of(const ENEmit &E, uint64_t i)
{
    ENWalk w{0, 0, 0, 0, 0, 0};
    if (i >= E.n) return w;
    const uint32_t cnt = E.len[i];
    const uint64_t cw = E.cell[i];
    if (!cnt || (cw & 0xFFu) != DG_TGET_OK) return w;
    w.o = E.off[i];
    if (w.o >= E.cap) return w; /* none of its slots is stored */
    w.p = E.val[i], w.e = w.p + E.span[i], w.left = cnt;
    w.kt = (uint32_t)(cw >> 32) & 0xFFu, w.vt = (uint32_t)(cw >> 40) & 0xFFu;
    return w;
}

/* variable stride, shape 1: one lane walks one cell and stores every entry as
 * it meets it; a store instruction of a wave touches 64 cells' slots */
__global__ __launch_bounds__(EN_BLOCK) void ents_emit_lane_kernel(ENEmit E)
{
    ENWalk w = en_walk_of(E, (uint64_t)blockIdx.x * EN_BLOCK + threadIdx.x);
    for (; w.left && w.o < E.cap; w.left--, w.o++) {
        ENEntry en;
        if (!en_next(E.src, w.p, w.e, E.kind, w.kt, w.vt, en)) break;
        en_put(E, w.o, en);
    }
}

/* variable stride, shape 2: a block is one wave. A round: every lane stages up
 * to R entries of its cell in its row of an LDS tile (rows R + 1 apart, so the
 * lanes' 8-byte columns fall on different banks); then lane t of step s takes
 * slot (s * 64 + t) % R of row (s * 64 + t) / R, so R neighbouring lanes cover
 * one cell's R neighbouring slots: runs of R * 8 bytes in key and v, R * 4 in
 * the lengths, instead of one slot per cell and instruction. */
template <uint32_t R>
__global__ __launch_bounds__(EN_WAVE) void ents_emit_stage_kernel(ENEmit E)
{
    constexpr uint32_t ROW = R + 1;
    __shared__ uint64_t skey[EN_WAVE * ROW], sval[EN_WAVE * ROW], sbase[EN_WAVE];
    __shared__ uint32_t sklen[EN_WAVE * ROW], svlen[EN_WAVE * ROW], scnt[EN_WAVE];
    const uint32_t t = threadIdx.x;
    ENWalk w = en_walk_of(E, (uint64_t)blockIdx.x * EN_WAVE + t);
    while (__syncthreads_or(w.left != 0)) { /* also: the previous round's tile is read */
        uint32_t k = 0;
        for (; k < R && w.left; k++, w.left--) {
            ENEntry en;
            if (!en_next(E.src, w.p, w.e, E.kind, w.kt, w.vt, en)) {
                w.left = 0;
                break;
            }
            skey[t * ROW + k] = en.key, sval[t * ROW + k] = en.val;
            sklen[t * ROW + k] = en.klen, svlen[t * ROW + k] = en.vlen;
        }
        scnt[t] = k, sbase[t] = w.o;
        w.o += k;
        __syncthreads();
#pragma unroll
        for (uint32_t s = 0; s < R; s++) {
            const uint32_t at = s * EN_WAVE + t, row = at / R, r = at % R;
            const uint64_t o = sbase[row] + r;
            if (r >= scnt[row] || o >= E.cap) continue;
            if (E.key) E.key[o] = skey[row * ROW + r];
            if (E.klen) E.klen[o] = sklen[row * ROW + r];
            if (E.v) E.v[o] = sval[row * ROW + r];
            if (E.vlen) E.vlen[o] = svlen[row * ROW + r];
        }
    }
}

void launch_ents_pass(hipStream_t s, const ENParams &A) { launch_walk<EntsOp>(s, A, A.tg.pairs); }

void launch_ents_emit(hipStream_t s, const ENEmit &E, uint32_t max_blocks, uint32_t stage)
{
    if ((E.kind & DG_ENT_INTMAP) && (E.kind & 15u) != DG_ENT_STR) { /* int keys and fixed-size values */
        const uint64_t chunks = (E.cap + EN_EMIT_CHUNK - 1) / EN_EMIT_CHUNK; /* no more entries than cap are stored */
        hipLaunchKernelGGL(ents_emit_fixed_kernel, dim3((uint32_t)(chunks < max_blocks ? chunks : max_blocks)),
                           dim3(EN_BLOCK), 0, s, E);
        return;
    }
    const dim3 waves((uint32_t)((E.n + EN_WAVE - 1) / EN_WAVE)), block(EN_WAVE);
    if (stage == 4) hipLaunchKernelGGL(ents_emit_stage_kernel<4>, waves, block, 0, s, E);
    else if (stage == 8) hipLaunchKernelGGL(ents_emit_stage_kernel<8>, waves, block, 0, s, E);
    else if (stage == 16) hipLaunchKernelGGL(ents_emit_stage_kernel<16>, waves, block, 0, s, E);
    else hipLaunchKernelGGL(ents_emit_lane_kernel, dim3((uint32_t)((E.n + EN_BLOCK - 1) / EN_BLOCK)), dim3(EN_BLOCK), 0, s, E);
}

}  // namespace dg
