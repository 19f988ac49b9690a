/*
 * flat_image.h — the flat kernel's per-descriptor image: everything a block
 * of j2t_flat_kernel copies to LDS that depends on the descriptor alone, in
 * the order it lies in LDS, so that the block's prologue is one pass of
 * 16-byte loads beside the JSON loads instead of a chain of table reads.
 *
 *   [0, blob16)            the descriptor blob, zero-padded to 16 bytes
 *   [blob16, +160)         p10u[20]   10^k as uint64, k = 0..19
 *   [.., +184)             p10d[23]   1e0 .. 1e22 as doubles (P10)
 *   [.., +8 * EL_WN)       the Eisel-Lemire window: DG_POW10_M128[EL_WLO + 348 + t][1]
 *   zero padding to 16 bytes
 *
 * Plain host code (no HIP): built once where the descriptor is created
 * (desc_finish, j2t_host.hip, through flat_image.hip), owned by the dg_desc.
 */
#pragma once
#include <stdint.h>
#include <string.h>

namespace dg {

constexpr int FLI_WLO = -40; /* = EL_WLO, EL_WN (j2t_fast.h asserts it) */
constexpr int FLI_WN = 64;
constexpr uint32_t FLI_NP10U = 20, FLI_NP10D = 23;
constexpr uint32_t FLI_P10U = 0;                              /* offsets of the tables behind the padded blob */
constexpr uint32_t FLI_P10D = FLI_P10U + 8 * FLI_NP10U;
constexpr uint32_t FLI_PW = FLI_P10D + 8 * FLI_NP10D;
constexpr uint32_t FLI_TABS = (FLI_PW + 8 * FLI_WN + 15) & ~15u; /* 864 */

/* 1e0 .. 1e22: the doubles P10 (j2t_device.h) holds */
static const double FLI_P10D_VALUES[FLI_NP10D] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

constexpr uint32_t fli_blob16(uint32_t total_len) { return (total_len + 15) & ~15u; }
constexpr uint32_t fli_len(uint32_t total_len) { return fli_blob16(total_len) + FLI_TABS; }

/* the image of blob[0, total_len) into img[0, fli_len(total_len)); pw_hi =
 * the table the window is cut from (DG_POW10_M128 as the host sees it) */
inline void fli_build(const uint8_t *blob, uint32_t total_len, const uint64_t (*pw_hi)[2], uint8_t *img)
{
    const uint32_t b16 = fli_blob16(total_len);
    memset(img, 0, fli_len(total_len));
    memcpy(img, blob, total_len);
    uint8_t *t = img + b16;
    uint64_t v = 1;
    for (uint32_t k = 0; k < FLI_NP10U; k++, v *= 10) memcpy(t + FLI_P10U + 8 * k, &v, 8);
    memcpy(t + FLI_P10D, FLI_P10D_VALUES, sizeof FLI_P10D_VALUES);
    for (int k = 0; k < FLI_WN; k++) memcpy(t + FLI_PW + 8 * k, &pw_hi[FLI_WLO + 348 + k][1], 8);
}

}  // namespace dg
