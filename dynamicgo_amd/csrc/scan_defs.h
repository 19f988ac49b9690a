/* scan_defs.h — the geometry of the scan of counts into offsets (scan_kern.h):
 * what a host needs to size the tile sums. No __global__ code. */
#pragma once
#include <stdint.h>

namespace dg {

constexpr uint32_t SCAN_BLOCK = 256;
constexpr uint32_t SCAN_TILE = 2048; /* counts a block takes, 8 a lane: one u64 of tile sums per SCAN_TILE counts */

}  // namespace dg
