// dm_photo.h -- device helpers shared by dm_photo.hip (dm_photo_score), dm_photo_refine.hip
// (dm_photo_refine) and dm_lsm.hip (dm_lsm_refine): rows of uint8 pixels read as unaligned dwords,
// and sums of products as chains of v_dot4_u32_u8.
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

// the first nbytes (4 .. 4 NW) bytes at p as NW little-endian dwords, zero from nbytes on.  Reads
// nothing outside [p, p + nbytes).
template <int NW>
__device__ __forceinline__ void pho_rowz(const uint8_t *p, int nbytes, uint32_t (&d)[NW])
{
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int left = nbytes - 4 * k;      // bytes of the row from dword k on
        if (left >= 4)
            d[k] = pho_ld4(p + 4 * k);
        else if (left > 0)
            d[k] = pho_ld4(p + nbytes - 4) >> (8 * (4 - left));
        else
            d[k] = 0u;
    }
}

// the bytes 0 .. 2r of a window row as a mask over its ND dwords
template <int ND>
__device__ __forceinline__ void pho_wmask(int D, uint32_t (&m)[ND])
{
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const int nb = D - 4 * k;      // bytes of the window in dword k: >= 1
        m[k] = nb >= 4 ? 0xffffffffu : (0xffffffffu >> (8 * (4 - nb)));
    }
}

// the window row that starts J bytes into raw (J a compile-time shift), cut to the mask
template <int J, int ND, int NW>
__device__ __forceinline__ void pho_shift(const uint32_t (&raw)[NW], const uint32_t (&m)[ND], uint32_t (&d)[ND])
{
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const int b = J + 4 * k, qd = b >> 2, rm = b & 3;
        const uint32_t lo = qd < NW ? raw[qd < NW ? qd : 0] : 0u;
        const uint32_t hi = qd + 1 < NW ? raw[qd + 1 < NW ? qd + 1 : 0] : 0u;
        d[k] = (rm ? ((lo >> (8 * rm)) | (hi << (32 - 8 * rm))) : lo) & m[k];
    }
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

// num and vb of dm_photo_score's rule 5 from the exact sums of one position: S[k] = sum P_k, A[k] =
// sum(A P_k), B = sum(P_k P_l) in the order 00 01 02 03 11 12 13 22 23 33
__device__ __forceinline__ void pho_numvb(int64_t n, int64_t Sa, const double (&w)[4], const uint32_t (&S)[4],
                                          const uint32_t (&A)[4], const uint32_t (&B)[10], double &num, double &vb)
{
    const int64_t s0 = S[0], s1 = S[1], s2 = S[2], s3 = S[3];
    const double CA0 = (double)(n * (int64_t)A[0] - Sa * s0), CA1 = (double)(n * (int64_t)A[1] - Sa * s1);
    const double CA2 = (double)(n * (int64_t)A[2] - Sa * s2), CA3 = (double)(n * (int64_t)A[3] - Sa * s3);
    const double C00 = (double)(n * (int64_t)B[0] - s0 * s0), C01 = (double)(n * (int64_t)B[1] - s0 * s1);
    const double C02 = (double)(n * (int64_t)B[2] - s0 * s2), C03 = (double)(n * (int64_t)B[3] - s0 * s3);
    const double C11 = (double)(n * (int64_t)B[4] - s1 * s1), C12 = (double)(n * (int64_t)B[5] - s1 * s2);
    const double C13 = (double)(n * (int64_t)B[6] - s1 * s3), C22 = (double)(n * (int64_t)B[7] - s2 * s2);
    const double C23 = (double)(n * (int64_t)B[8] - s2 * s3), C33 = (double)(n * (int64_t)B[9] - s3 * s3);
    num = ((w[0] * CA0 + w[1] * CA1) + w[2] * CA2) + w[3] * CA3;
    vb = (1.0 * (w[0] * w[0])) * C00;
    vb = vb + (2.0 * (w[0] * w[1])) * C01;
    vb = vb + (2.0 * (w[0] * w[2])) * C02;
    vb = vb + (2.0 * (w[0] * w[3])) * C03;
    vb = vb + (1.0 * (w[1] * w[1])) * C11;
    vb = vb + (2.0 * (w[1] * w[2])) * C12;
    vb = vb + (2.0 * (w[1] * w[3])) * C13;
    vb = vb + (1.0 * (w[2] * w[2])) * C22;
    vb = vb + (2.0 * (w[2] * w[3])) * C23;
    vb = vb + (1.0 * (w[3] * w[3])) * C33;
}

// the score of rule 5 from VA, num and vb
__device__ __forceinline__ double pho_zncc(double VA, double num, double vb)
{
    if (VA > 0.0 && vb > 0.0) {
        const double t = num / sqrt(VA * vb);
        return t > 1.0 ? 1.0 : (t < -1.0 ? -1.0 : t);
    }
    return 0.0;
}

#endif // DM_PHOTO_H
