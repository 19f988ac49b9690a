/* The flat kernel's per-descriptor image, built on the host (flat_image.h).
 * This unit holds host code only and reads the powers-of-ten table as a host
 * array: under hipcc dg_tables.h declares it __device__ __constant__, whose
 * host-side shadow carries no values, so the two attributes are defined away
 * before the table is included (no HIP header follows). The values are the
 * ones every kernel reads: the same header. */
#include <stdint.h>

#undef __device__
#define __device__
#undef __constant__
#define __constant__
#include "dg_tables.h"
#include "flat_image.h"

namespace dg {
void flat_image_build(const uint8_t *blob, uint32_t total_len, uint8_t *img)
{
    fli_build(blob, total_len, DG_POW10_M128, img);
}
}  // namespace dg
