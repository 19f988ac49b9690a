/* rows kernels (row columns, rows_device.h): the head and index passes and the
 * row cell pass, each with its deep pass. The scan between them is cols'. */
#include "rows_device.h"

namespace dg {

/* One lane per message, kids_kernel<0>'s geometry. INDEX 0: the head/count
 * pass. INDEX 1: the index pass. Messages nested beyond the LDS levels are
 * queued for rows_msg_deep_kernel. */
template <int INDEX>
__global__ __launch_bounds__(RW_BLOCK) void rows_msg_kernel(RWParams A)
{
    __shared__ uint64_t lf[TG_LDS_DEPTH * TG_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (i >= A.n) return;
    const RWLdsFrames fr{{&lf[threadIdx.x]}};
    const bool deep = INDEX ? rw_index_msg(A, i, fr) : rw_head_msg(A, i, fr);
    if (deep) A.deep_list[atomicAdd(A.cnt, 1u)] = (uint32_t)i;
}

/* the queued messages again from the start with TG_DEEP_DEPTH levels per lane
 * in device memory; also zeroes the counter the previous pass used */
template <int INDEX>
__global__ __launch_bounds__(TG_DEEP_BLOCK) void rows_msg_deep_kernel(RWParams A)
{
    const uint32_t cnt = *(volatile const uint32_t *)A.cnt;
    const uint32_t lane = blockIdx.x * TG_DEEP_BLOCK + threadIdx.x;
    if (lane == 0) *A.reset = 0;
    const RWDeepFrames fr{{A.ws + lane}};
    for (uint32_t g = lane; g < cnt; g += TG_DEEP_LANES) {
        const uint64_t i = A.deep_list[g];
        if (INDEX) (void)rw_index_msg(A, i, fr);
        else if (rw_head_msg(A, i, fr)) /* unreachable: 1023 levels fit */
            rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps);
    }
}

/* The row cell pass: one lane per (row, column) pair, the P pairs of a row in
 * neighbouring lanes (cols_kernel's geometry over rows). The grid covers
 * row_cap * P pairs; the rows there are come from row_off[n]. Stores are
 * column-major, so a wave writes contiguous runs in each column. */
__global__ __launch_bounds__(RW_BLOCK) void rows_kernel(RWParams A)
{
    __shared__ uint64_t lf[TG_LDS_DEPTH * TG_BLOCK];
    const uint64_t q = (uint64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const uint32_t P = A.sub.P;
    if (q >= rw_rows(A) * P) return;
    const uint64_t g = q / P;
    const uint32_t k = (uint32_t)(q - g * P);
    const RWLdsFrames fr{{&lf[threadIdx.x]}};
    const CLCell c = rw_cell(A, g, k, fr);
    if (c.status == TG_ST_DEEP) {
        A.deep_list[atomicAdd(A.cnt, 1u)] = (uint32_t)q;
        return;
    }
    rw_store(A, g, k, c);
}

__global__ __launch_bounds__(TG_DEEP_BLOCK) void rows_deep_kernel(RWParams A)
{
    const uint32_t cnt = *(volatile const uint32_t *)A.cnt;
    const uint32_t lane = blockIdx.x * TG_DEEP_BLOCK + threadIdx.x;
    if (lane == 0) *A.reset = 0;
    const uint32_t P = A.sub.P;
    const RWDeepFrames fr{{A.ws + lane}};
    for (uint32_t t = lane; t < cnt; t += TG_DEEP_LANES) {
        const uint64_t q = A.deep_list[t];
        const uint64_t g = q / P;
        const uint32_t k = (uint32_t)(q - g * P);
        CLCell c = rw_cell(A, g, k, fr);
        if (c.status == TG_ST_DEEP) c.status = DG_TGET_E_READ; /* unreachable: 1023 levels fit */
        rw_store(A, g, k, c);
    }
}

void launch_rows_head(hipStream_t s, const RWParams &A)
{
    hipLaunchKernelGGL(rows_msg_kernel<0>, dim3((uint32_t)((A.n + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, s, A);
    hipLaunchKernelGGL(rows_msg_deep_kernel<0>, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

void launch_rows_index(hipStream_t s, const RWParams &A)
{
    hipLaunchKernelGGL(rows_msg_kernel<1>, dim3((uint32_t)((A.n + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, s, A);
    hipLaunchKernelGGL(rows_msg_deep_kernel<1>, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

void launch_rows_cells(hipStream_t s, const RWParams &A)
{
    const uint64_t pairs = A.row_cap * A.sub.P;
    hipLaunchKernelGGL(rows_kernel, dim3((uint32_t)((pairs + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, s, A);
    hipLaunchKernelGGL(rows_deep_kernel, dim3(TG_DEEP_BLOCKS), dim3(TG_DEEP_BLOCK), 0, s, A);
}

}  // namespace dg
