/*
 * host_layout.h — the arithmetic of one host batch, shared by the host entries
 * of tget, cut, edit, editm, kids and t2j (HostBatch, host_internal.h): offsets
 * rebased to 0, 16-byte slots, the gather of a rerun, value offsets. Plain
 * C++17 and no HIP type, so a CPU program can include it
 * (tests/host_layout_host.cpp). Every array is the caller's, of exactly the
 * size named; a refusal writes nothing past the entry it refuses. A batch is
 * 65 536 messages and a host entry is timed in microseconds, so each routine is
 * one pass that keeps its running values in registers.
 */
#pragma once
#include <stdint.h>

#include <algorithm>

namespace dg {

enum : int { HL_OK = 0, HL_DESCENDING = 1, HL_TOO_LONG = 2 };
constexpr uint64_t HL_SLOT_MAX = 0xFFFFFFFFull; /* out_len is 32 bits wide */

/* The messages idx[0..m) of in_off (idx null: the messages 0..m) laid back to
 * back: io[m + 1] from 0, *longest (optional) = the longest one, src[m]
 * (optional) = where each starts in the caller's arena. With so (optional): so[m + 1], a
 * slot of cap_of(i, len) bytes for message i of len bytes, rounded up to 16
 * (the packing reads its slots as aligned words).
 * Refused, with *bad = the message: in_off[i + 1] < in_off[i] (HL_DESCENDING),
 * a capacity over HL_SLOT_MAX (HL_TOO_LONG, *bad_cap = the capacity). */
template <class F>
inline int hl_layout(const uint64_t *in_off, const uint64_t *idx, uint64_t m, F cap_of, uint64_t *io, uint64_t *so,
                     uint64_t *src, uint64_t *longest, uint64_t *bad, uint64_t *bad_cap)
{
    uint64_t in_at = io[0] = 0, out_at = 0, most = 0;
    if (so) so[0] = 0;
    int rc = HL_OK;
    for (uint64_t k = 0; k < m; k++) {
        const uint64_t i = idx ? idx[k] : k, a = in_off[i], b = in_off[i + 1], len = b - a;
        if (b < a) {
            rc = HL_DESCENDING, *bad = i;
            break;
        }
        if (so) {
            const uint64_t cap = cap_of(i, len);
            if (cap > HL_SLOT_MAX) {
                rc = HL_TOO_LONG, *bad = i, *bad_cap = cap;
                break;
            }
            so[k + 1] = out_at += (cap + 15) & ~15ull;
        }
        if (src) src[k] = a;
        io[k + 1] = in_at += len;
        if (longest) most = std::max(most, len); /* a dependent chain of its own: not for a caller without use for it */
    }
    if (longest) *longest = most;
    return rc;
}

/* off[count + 1] ascending -> rel[count + 1] = off[] - off[0]; longest[q % K]
 * (K entries, K >= 1) = the longest span of its residue: edit's values are
 * K = 1, editm's message-major ones count = n K */
inline int hl_rebase(const uint64_t *off, uint64_t count, uint64_t K, uint64_t *rel, uint64_t *longest)
{
    std::fill(longest, longest + K, 0);
    rel[0] = 0;
    for (uint64_t q = 0, j = 0; q < count; q++, j = j + 1 == K ? 0 : j + 1) { /* j = q % K without the division */
        if (off[q + 1] < off[q]) return HL_DESCENDING;
        rel[q + 1] = off[q + 1] - off[0];
        longest[j] = std::max(longest[j], off[q + 1] - off[q]);
    }
    return HL_OK;
}

}  // namespace dg
