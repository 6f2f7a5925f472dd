// dm_photo.h -- what the four stages that read the image pair share: dm_photo.hip (dm_photo_score),
// dm_photo_refine.hip (dm_photo_refine), dm_lsm.hip (dm_lsm_refine) and dm_sgm.hip (dm_sgm_refine).
// dm_lsm_affine.hip (dm_lsm_affine), the affine model of the lsm stage, uses the host side, pho_cell,
// pho_bilin, pho_numvb and pho_zncc.
//
// Host side, used by all four entries:
//   pho_pair_args   the argument checks they have in common (image shape, strides, map shape, offset,
//                   radius), in that order, with their messages
//   pho_pair_plan   the shapes a plane re-matching entry takes (refine, lsm, sgm)
//   pho_grid, PHO_SWITCH_ND   the launch grid of one thread per cell and the dispatch on ND = (radius + 2) / 2
// Device side:
//   pho_cell        the cell of a thread (k_photo, k_refine, k_lsm, k_sgm_cost, k_sgm_pick)
//   pho_row, pho_rowz, pho_shift, pho_wmask   rows of uint8 pixels read as unaligned dwords and cut into
//                   shifted window rows (all four; the 3-byte case of pho_rowz is k_sgm_cost's)
//   pho_dot, pho_sum   sums of products as chains of v_dot4_u32_u8 (all four)
//   pho_moments1    sum A and sum A^2 of the img1 window (k_refine, k_sgm_cost)
//   pho_bilin       a position as its integer corner and bilinear weights (k_photo, k_refine, k_lsm)
//   pho_numvb, pho_zncc   the float64 tail of dm_photo_score's rule 5 (k_photo, k_refine, k_lsm; pho_zncc
//                   also k_sgm_cost and k_sgm_pick)
#ifndef DM_PHOTO_H
#define DM_PHOTO_H

#include "dm_host.h"      // dm_is_hole, dm_nan; dm_fail and dm_maps_plan for the entries

#define PHO_TX 32
#define PHO_TY 8
#define PHO_RMAX 7
#define PHO_OFFMAX (1 << 30)

// ---- host side ------------------------------------------------------------------------------
// the checks every entry makes on the pair, the map and the window: DM_OK, or the code of the first that fails
__attribute__((unused)) static int pho_pair_args(int64_t stride1, int64_t stride2, int32_t Hi, int32_t Wi, int32_t H,
                                                 int32_t W, int32_t oy, int32_t ox, int32_t radius)
{
    if (Hi < 1 || Wi < 1) return dm_fail(DM_ERR_ARG, "bad image shape Hi=%d Wi=%d", Hi, Wi);
    if (stride1 < Wi || stride2 < Wi)
        return dm_fail(DM_ERR_ARG, "row stride below the image width %d (got %lld, %lld)", Wi, (long long)stride1,
                     (long long)stride2);
    if (H < 1 || W < 1) return dm_fail(DM_ERR_ARG, "bad map shape H=%d W=%d", H, W);
    if (oy < -PHO_OFFMAX || oy > PHO_OFFMAX || ox < -PHO_OFFMAX || ox > PHO_OFFMAX)
        return dm_fail(DM_ERR_ARG, "offset must be in [-2^30, 2^30] (got %d, %d)", oy, ox);
    if (radius < 1 || radius > PHO_RMAX) return dm_fail(DM_ERR_ARG, "radius must be in [1, %d] (got %d)", PHO_RMAX, radius);
    return DM_OK;
}

// false for a shape the plane re-matching entries do not take (dm_photo_bytes' limits, and images of at most
// 2^30 a side)
__attribute__((unused)) static bool pho_pair_plan(int32_t Hi, int32_t Wi, int32_t H, int32_t W)
{
    if (Hi < 1 || Wi < 1 || Hi > (1 << 30) || Wi > (1 << 30)) return false;
    return dm_photo_bytes(1, H, W) != 0;
}

// the grid of one thread per cell: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells (tiles_x tiles_y < 2^31)
__attribute__((unused)) static dim3 pho_grid(int32_t H, int32_t W, int *tiles_x)
{
    const int tiles_y = (H + PHO_TY - 1) / PHO_TY;
    *tiles_x = (W + PHO_TX - 1) / PHO_TX;
    return dim3((unsigned)*tiles_x * (unsigned)tiles_y);
}

// GO(ND) for the ND = (radius + 2) / 2 dwords of a window row of 2 radius + 1 bytes
#define PHO_SWITCH_ND(radius, GO) \
    switch (((radius) + 2) / 2) { \
    case 1: GO(1); break;         \
    case 2: GO(2); break;         \
    case 3: GO(3); break;         \
    default: GO(4); break;        \
    }

// ---- device side ----------------------------------------------------------------------------
// the cell (y, x) of this thread in a pho_grid launch; false outside the map
__device__ __forceinline__ bool pho_cell(int tiles_x, int H, int W, int &y, int &x)
{
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    y = tile_y * PHO_TY + (int)(threadIdx.x / PHO_TX), x = tile_x * PHO_TX + (int)(threadIdx.x % PHO_TX);
    return y < H && x < W;
}

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

// the first nbytes (4 .. 4 NW; with B3 3 .. 4 NW) bytes at p as NW little-endian dwords, zero from nbytes
// on.  Reads nothing outside [p, p + nbytes).
template <int NW, bool B3 = false>
__device__ __forceinline__ void pho_rowz(const uint8_t *p, int nbytes, uint32_t (&d)[NW])
{
    if (B3 && nbytes < 4) {
        d[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
#pragma unroll
        for (int k = 1; k < NW; ++k) d[k] = 0u;
        return;
    }
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

// sum A and sum A^2 of the img1 window whose top-left byte is pa
template <int ND>
__device__ __forceinline__ void pho_moments1(const uint8_t *pa, size_t stride1, int D, const uint32_t (&wmask)[ND],
                                             uint32_t &sa, uint32_t &saa)
{
    sa = 0, saa = 0;
    for (int q = 0; q < D; ++q) {
        uint32_t ac[ND];
        pho_row<ND>(pa + (size_t)q * stride1, D, ac);
#pragma unroll
        for (int k = 0; k < ND; ++k) ac[k] &= wmask[k];
        sa = pho_sum<ND>(ac, sa);
        saa = pho_dot<ND>(ac, ac, saa);
    }
}

// a position (converted only after its caller tested it in double) as its integer corner and the bilinear
// weights of the four pixels (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1).  Returned by value: with
// iy and ix as reference parameters the compiler orders k_photo's window tests differently.
struct PhoPos {
    int iy, ix;
    double w[4];
};

__device__ __forceinline__ PhoPos pho_bilin(double py, double px)
{
    const double fly = floor(py), flx = floor(px);
    const int iy = (int)fly, ix = (int)flx;
    const double fy = py - fly, fx = px - flx;
    const double gy = 1.0 - fy, gx = 1.0 - fx;
    return {iy, ix, {gy * gx, gy * fx, fy * gx, fy * fx}};
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
