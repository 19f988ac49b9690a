/* rows kernels (row columns, rows_device.h): the head, index and row cell
 * passes, three operations of the pair pass (walk_kern.h), and the map plans'
 * head and index passes, two more. The scan between them is cols'. */
#include "rows_device.h"
#include "walk_kern.h"

namespace dg {

static_assert(RW_BLOCK == TG_BLOCK, "the pair pass's block");

struct RowsOp {
    using Params = RWParams;
    using Lds = RWLdsFrames;
    using Deep = RWDeepFrames;
    static __device__ __forceinline__ WalkQueue queue(const RWParams &A) { return WalkQueue{A.deep_list, A.cnt, A.reset, A.ws}; }
};

/* The head/count pass: one lane per message, a pair pass of one "column" (a
 * compile-time 1: the pair is the message). The lane pass calls rw_head_msg
 * itself (walk_kern.h says why). */
struct RowsHeadOp : RowsOp {
    static __device__ __forceinline__ uint64_t pairs(const RWParams &A) { return A.n; }
    template <class FR>
    static constexpr bool (*lane)(const RWParams &, uint64_t, const FR &) = &rw_head_msg<FR>;
    template <class FR>
    static __device__ __forceinline__ void deep(const RWParams &A, uint64_t i, const FR &fr)
    {
        if (rw_head_msg(A, i, fr)) rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps); /* unreachable: 1023 levels fit */
    }
};

/* the index pass: one lane per message; a walk still deep in the deep pass
 * (unreachable) stores nothing */
struct RowsIndexOp : RowsOp {
    static __device__ __forceinline__ uint64_t pairs(const RWParams &A) { return A.n; }
    template <class FR>
    static constexpr bool (*lane)(const RWParams &, uint64_t, const FR &) = &rw_index_msg<FR>;
    template <class FR>
    static constexpr bool (*deep)(const RWParams &, uint64_t, const FR &) = &rw_index_msg<FR>;
};

/* The row cell pass: pair q = (row q / P, column q % P), the P pairs of a row
 * in neighbouring lanes (cols' geometry over rows). The grid covers row_cap * P
 * pairs; the rows there are come from row_off[n]. Stores are column-major, so
 * a wave writes contiguous runs in each column. */
struct RowsCellOp : RowsOp {
    static __device__ __forceinline__ uint64_t pairs(const RWParams &A) { return rw_rows(A) * A.sub.P; }
    template <class FR>
    static __device__ __forceinline__ bool pair(const RWParams &A, uint64_t q, const FR &fr, bool last)
    {
        const uint32_t P = A.sub.P;
        const uint64_t g = q / P;
        const uint32_t k = (uint32_t)(q - g * P);
        CLCell c = rw_cell(A, g, k, fr);
        if (c.status == TG_ST_DEEP) {
            if (!last) return true;
            c.status = DG_TGET_E_READ; /* unreachable: 1023 levels fit */
        }
        rw_store(A, g, k, c);
        return false;
    }
    template <class FR>
    static __device__ __forceinline__ bool lane(const RWParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, false); }
    template <class FR>
    static __device__ __forceinline__ bool deep(const RWParams &A, uint64_t q, const FR &fr) { return pair(A, q, fr, true); }
};

/* The map plans' head and index passes: the same geometry over RWMapParams.
 * Operations of their own, so the list kernels above are instantiated from
 * exactly the code they were. */
struct RowsMapOp : RowsOp {
    using Params = RWMapParams;
    static __device__ __forceinline__ uint64_t pairs(const RWMapParams &A) { return A.n; }
};
struct RowsMapHeadOp : RowsMapOp {
    template <class FR>
    static constexpr bool (*lane)(const RWMapParams &, uint64_t, const FR &) = &rw_map_head_msg<FR>;
    template <class FR>
    static __device__ __forceinline__ void deep(const RWMapParams &A, uint64_t i, const FR &fr)
    {
        if (rw_map_head_msg(A, i, fr)) rw_put_head(A, i, 0, 0, DG_TGET_E_READ, 0, 0, A.n_steps); /* unreachable: 1023 levels fit */
    }
};
struct RowsMapIndexOp : RowsMapOp {
    template <class FR>
    static constexpr bool (*lane)(const RWMapParams &, uint64_t, const FR &) = &rw_map_index_msg<FR>;
    template <class FR>
    static constexpr bool (*deep)(const RWMapParams &, uint64_t, const FR &) = &rw_map_index_msg<FR>;
};

void launch_rows_map_head(hipStream_t s, const RWMapParams &A) { launch_walk<RowsMapHeadOp>(s, A, A.n); }

void launch_rows_map_index(hipStream_t s, const RWMapParams &A) { launch_walk<RowsMapIndexOp>(s, A, A.n); }

void launch_rows_head(hipStream_t s, const RWParams &A) { launch_walk<RowsHeadOp>(s, A, A.n); }

void launch_rows_index(hipStream_t s, const RWParams &A) { launch_walk<RowsIndexOp>(s, A, A.n); }

void launch_rows_cells(hipStream_t s, const RWParams &A) { launch_walk<RowsCellOp>(s, A, A.row_cap * A.sub.P); }

}  // namespace dg
