// dm_photo.h -- device helpers shared by dm_photo.hip (dm_photo_score) and dm_photo_refine.hip
// (dm_photo_refine): rows of uint8 pixels read as unaligned dwords, and sums of products as
// chains of v_dot4_u32_u8.
#ifndef DM_PHOTO_H
#define DM_PHOTO_H

#include "dm_host.h"      // dm_is_hole; dm_fail and dm_maps_plan for the two entries

#define PHO_TX 32
#define PHO_TY 8
#define PHO_RMAX 7
#define PHO_OFFMAX (1 << 30)

__device__ __forceinline__ bool pho_finite(double x) { return !dm_is_hole(x); }

__device__ __forceinline__ uint32_t pho_ld4(const uint8_t *p)      // a dword at any byte address
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// the first nbytes (3 .. 4 ND) bytes at p as ND little-endian dwords; the bytes from nbytes on are
// arbitrary.  Reads nothing outside [p, p + nbytes).
template <int ND>
__device__ __forceinline__ void pho_row(const uint8_t *p, int nbytes, uint32_t (&d)[ND])
{
    if (ND == 1 && nbytes < 4) {
        d[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        return;
    }
#pragma unroll
    for (int k = 0; k < ND - 1; ++k) d[k] = pho_ld4(p + 4 * k);
    const int rem = nbytes - 4 * (ND - 1);                       // 1 .. 4 bytes in the last dword
    d[ND - 1] = pho_ld4(p + nbytes - 4) >> (8 * (4 - rem));
}

template <int ND>
__device__ __forceinline__ uint32_t pho_dot(const uint32_t (&a)[ND], const uint32_t (&b)[ND], uint32_t acc)
{
#pragma unroll
    for (int k = 0; k < ND; ++k) acc = __builtin_amdgcn_udot4(a[k], b[k], acc, false);
    return acc;
}

template <int ND>
__device__ __forceinline__ uint32_t pho_sum(const uint32_t (&a)[ND], uint32_t acc)
{
#pragma unroll
    for (int k = 0; k < ND; ++k) acc = __builtin_amdgcn_udot4(a[k], 0x01010101u, acc, false);
    return acc;
}

#endif // DM_PHOTO_H
