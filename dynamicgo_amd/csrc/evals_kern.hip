/* evals kernels (entry column writes, evals_device.h): the entry-size pass of a
 * variable-stride column, the cell pass, the head pass and the entry-parallel
 * emit. The scans between them are cols', the offsets' shift to out_base vals'. */
#include "evals_device.h"

namespace dg {

/* One lane per entry of a variable-stride column: its encoded bytes for the
 * scan. Lengths alone are read, and none at an index >= n_ent. */
__global__ __launch_bounds__(EV_BLOCK) void evals_entry_size_kernel(const uint32_t *key_len, const uint32_t *val_len,
                                                                    uint64_t n_ent, uint32_t kt, uint32_t vt, uint32_t *elen)
{
    const uint64_t g = (uint64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (g >= n_ent) return;
    elen[g] = ev_entry_size(kt, vt, kt == TT_STRING ? key_len[g] : 0u, vt == TT_STRING ? val_len[g] : 0u);
}

/* One lane per cell, the K cells of a message in neighbouring lanes: the
 * item's length and the count to emit for the two scans, and the status. */
__global__ __launch_bounds__(EV_BLOCK) void evals_cell_kernel(EVParams A)
{
    const uint64_t q = (uint64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (q >= A.pairs) return;
    const EVCell z = ev_pair_cell(A, ev_pair(A, q));
    A.len[q] = z.len, A.cnt[q] = z.cnt;
    if (A.status) A.status[q] = (uint8_t)z.status;
}

/* One lane per cell: what precedes the entries, and STOP. */
__global__ __launch_bounds__(EV_BLOCK) void evals_head_kernel(EVParams A)
{
    const uint64_t q = (uint64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (q >= A.pairs) return;
    const EVPair p = ev_pair(A, q);
    const uint64_t pos = A.off[q];
    ev_head(p.kind, p.id, p.fh, p.stop, (uint32_t)(A.off[q + 1] - pos), A.cnt[q], A.out, pos, A.cap);
}

/* The emit, in cols_emit_kernel's geometry over the scanned counts of all
 * cells: a block takes EV_CHUNK neighbouring emitted entries a round, its first
 * and last lane search all cells for the chunk's first and last entry, and in
 * step r lane t takes entry base + r * EV_BLOCK + t and searches between the
 * two answers. Neighbouring lanes write neighbouring entries of the arena. */
__global__ __launch_bounds__(EV_BLOCK) void evals_emit_kernel(EVParams A)
{
    __shared__ uint64_t range[2];
    const uint64_t total = A.cnt_off[A.pairs];
    for (uint64_t base = (uint64_t)blockIdx.x * EV_CHUNK; base < total; base += (uint64_t)gridDim.x * EV_CHUNK) {
        const uint64_t end = base + EV_CHUNK < total ? base + EV_CHUNK : total;
        if (threadIdx.x == 0) range[0] = cl_find(A.cnt_off, 0, A.pairs, base);
        if (threadIdx.x == EV_BLOCK - 1) range[1] = cl_find(A.cnt_off, 0, A.pairs, end - 1);
        __syncthreads();
        const uint64_t lo = range[0], hi = range[1] + 1;
        __syncthreads(); /* the next round writes range again */
        for (uint64_t t = base + threadIdx.x; t < end; t += EV_BLOCK) ev_emit(A, cl_find(A.cnt_off, lo, hi, t), t);
    }
}

static_assert(EV_BLOCK == VL_BLOCK, "cell_grid (vals_device.h) counts in blocks of VL_BLOCK");

void launch_evals_entry_size(hipStream_t s, const dg_eval_col &c, uint32_t kt, uint32_t vt, uint32_t *elen)
{
    hipLaunchKernelGGL(evals_entry_size_kernel, dim3((uint32_t)((c.n_ent + EV_BLOCK - 1) / EV_BLOCK)), dim3(EV_BLOCK), 0, s,
                       c.d_key_len, c.d_val_len, c.n_ent, kt, vt, elen);
}

void launch_evals_cells(hipStream_t s, const EVParams &A) { hipLaunchKernelGGL(evals_cell_kernel, cell_grid(A.pairs), dim3(EV_BLOCK), 0, s, A); }

void launch_evals_emit(hipStream_t s, const EVParams &A, uint32_t blocks)
{
    hipLaunchKernelGGL(evals_head_kernel, cell_grid(A.pairs), dim3(EV_BLOCK), 0, s, A);
    if (blocks) hipLaunchKernelGGL(evals_emit_kernel, dim3(blocks), dim3(EV_BLOCK), 0, s, A);
}

}  // namespace dg
