// dm_lsm_affine.hip -- gfx950 kernel + C ABI of the affine least-squares matching of a disparity map
// (dm_lsm_affine, include/dmstereo_lsm.h): every cell linearises img1 around its window (doubled
// central differences Gx, Gy) and solves, `iters` times, the 6 x 6 normal equations for the affine
// warp -- shift, stretch and shear on both axes -- that best explains the window of img1 by img2
// sampled under the warp, gain and offset left free.  The result is kept only if the correlation
// under the final warp is above dm_photo_score's at the start.
//
// k_lsm_affine: one launch, one thread per cell, workgroups of 32 x 8 cells (dm_photo.h).
//   staging         the tile of img1 with its r + 1 halo, at most 24 x 48 bytes, is written to LDS
//                   once; a pixel outside the image is staged as 0 and never used: a cell whose halo
//                   window leaves the image is skipped (rule 1).
//   once per cell   lsa_moments: one walk over the window in LDS; the six regressors of a tap are
//                   rebuilt from five bytes, the 21 + 6 + 6 + 2 sums are int32 (|phi| <= 1785, so
//                   sum(phi^2) <= 225 * 1785^2 < 2^30), combined in int64 and converted exactly.
//                   lsa_factor: N = L D L^T, unrolled; lsa_start: dm_photo_score's score at the
//                   start from the exact sums over the four integer windows (pho_numvb, pho_zncc).
//   each step       lsa_sums<true>: one walk over the taps; a tap reads its img1 bytes from LDS and
//                   its four img2 pixels from global memory as two unaligned 16-bit loads, forms
//                   the bilinear sample and adds to the nine float64 sums in raster order.
//   at the end      lsa_sums<false>: the three sums of the score under the final warp.
// Nothing is indexed dynamically: the factors, moments, sums and parameters live in registers.
//
// Reads: a tap's corner (iy, ix) comes from a warp whose four corner taps passed 0 <= Y < Hi - 1 and
// 0 <= X < Wi - 1 in double; the taps between them lie between (rounding is monotone in u and in
// v).  The converted corner is clamped to [0, Hi - 2] x [0, Wi - 2] all the same, which changes
// nothing and keeps the four pixels inside the image whatever the arithmetic does.  The start score
// reads the patch that dm_photo_score's rule 3 admits.  A cell reads only its own d_row / d_col and
// does so before it writes, so the outputs may alias the inputs.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "../../include/dmstereo_lsm.h"
#include "dm_photo.h"

#define LSA_ITMAX 8
#define LSA_RMIN 2
#define LSA_TW (PHO_TX + 2 * (PHO_RMAX + 1))
#define LSA_TH (PHO_TY + 2 * (PHO_RMAX + 1))

#define LSA_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))        // N_ij, c_ij: i >= j
#define LSA_LOW(i, j) ((i) * ((i)-1) / 2 + (j))          // L_ij: i > j

struct LsaCell {
    double sa, VA, n;
    double f[6], RA[6];
    double L[15], d[6];
};

__device__ __forceinline__ uint32_t lsa_ld2(const uint8_t *p)      // two bytes at any address
{
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// rule 2 and rule 3: t is the cell's centre in the staged tile, tw the tile's row pitch.  false: a pivot failed
__device__ __forceinline__ bool lsa_moments_factor(const uint8_t *t, int tw, int r, LsaCell &m)
{
    int f[6], RA[6], M[21], sa = 0, saa = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = RA[k] = 0;
#pragma unroll
    for (int k = 0; k < 21; ++k) M[k] = 0;
    for (int v = -r; v <= r; ++v) {
        const uint8_t *row = t + v * tw;
        int aL = row[-r - 1], aC = row[-r];
        for (int u = -r; u <= r; ++u) {
            const int aR = row[u + 1];
            const int gx = aR - aL, gy = (int)row[u + tw] - (int)row[u - tw];
            const int phi[6] = {gx, gx * u, gx * v, gy, gy * u, gy * v};
            sa += aC, saa += aC * aC;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                f[k] += phi[k];
                RA[k] += phi[k] * aC;
#pragma unroll
                for (int l = 0; l <= k; ++l) M[LSA_TRI(k, l)] += phi[k] * phi[l];
            }
            aL = aC, aC = aR;
        }
    }
    const int D = 2 * r + 1;
    const int64_t n = (int64_t)D * D;
    m.n = (double)n;
    m.sa = (double)sa;
    m.VA = (double)(n * (int64_t)saa - (int64_t)sa * sa);
    double N[21], c[21];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        m.f[k] = (double)f[k];
        m.RA[k] = (double)(n * (int64_t)RA[k] - (int64_t)f[k] * sa);
#pragma unroll
        for (int l = 0; l <= k; ++l) N[LSA_TRI(k, l)] = (double)(n * (int64_t)M[LSA_TRI(k, l)] - (int64_t)f[k] * f[l]);
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int i = j; i < 6; ++i) {
            double cij = N[LSA_TRI(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) cij = cij - m.L[LSA_LOW(i, k)] * c[LSA_TRI(j, k)];
            c[LSA_TRI(i, j)] = cij;
        }
        m.d[j] = c[LSA_TRI(j, j)];
        ok = ok && (m.d[j] > N[LSA_TRI(j, j)] * 0x1p-20);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) m.L[LSA_LOW(i, j)] = c[LSA_TRI(i, j)] / m.d[j];
    }
    return ok;
}

// rule 4: dm_photo_score's score at a start that passed its rule 3
__device__ __forceinline__ double lsa_start(const uint8_t *t, int tw, const uint8_t *img2, size_t stride2, int r,
                                            double py0, double px0, const LsaCell &m)
{
    const PhoPos pos = pho_bilin(py0, px0);
    uint32_t S[4], A[4], B[10];
#pragma unroll
    for (int k = 0; k < 4; ++k) S[k] = A[k] = 0;
#pragma unroll
    for (int k = 0; k < 10; ++k) B[k] = 0;
    for (int v = -r; v <= r; ++v) {
        const uint8_t *q = img2 + (size_t)(pos.iy + v) * stride2 + pos.ix;
        for (int u = -r; u <= r; ++u) {
            const uint32_t lo = lsa_ld2(q + u), hi = lsa_ld2(q + stride2 + u), a = t[v * tw + u];
            const uint32_t p[4] = {lo & 0xffu, lo >> 8, hi & 0xffu, hi >> 8};
            int b = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                S[k] += p[k];
                A[k] += a * p[k];
#pragma unroll
                for (int l = k; l < 4; ++l) B[b++] += p[k] * p[l];
            }
        }
    }
    double num, vb;
    pho_numvb((int64_t)m.n, (int64_t)m.sa, pos.w, S, A, B, num, vb);
    return pho_zncc(m.VA, num, vb);
}

// the corner test of rule 5 on the parameters p = (px, a, b, py, c, d); a NaN fails
__device__ __forceinline__ bool lsa_warp_ok(const double (&p)[6], int r, int Hi, int Wi)
{
    const double a1 = 1.0 + p[1], d1 = 1.0 + p[5], xmax = (double)(Wi - 1), ymax = (double)(Hi - 1);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double u = (double)((k & 1) ? r : -r), v = (double)((k & 2) ? r : -r);
        const double X = p[0] + (a1 * u + p[2] * v), Y = p[3] + (p[4] * u + d1 * v);
        ok = ok && (Y >= 0.0 && Y < ymax && X >= 0.0 && X < xmax);
    }
    return ok;
}

// the sums of a warp that passed lsa_warp_ok (rule 5), T only with GRAD
template <bool GRAD>
__device__ __forceinline__ void lsa_sums(const uint8_t *t, int tw, const uint8_t *img2, size_t stride2, int Hi, int Wi,
                                         int r, const double (&p)[6], double &Sp, double &Spp, double &Sap,
                                         double (&T)[6])
{
    const double a1 = 1.0 + p[1], d1 = 1.0 + p[5];
    Sp = Spp = Sap = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) T[k] = 0.0;
    for (int v = -r; v <= r; ++v) {
        const uint8_t *row = t + v * tw;
        const double dv = (double)v, bv = p[2] * dv, d1v = d1 * dv;
        int aL = row[-r - 1], aC = row[-r];
        for (int u = -r; u <= r; ++u) {
            const double du = (double)u;
            const double X = p[0] + (a1 * du + bv), Y = p[3] + (p[4] * du + d1v);
            const PhoPos pos = pho_bilin(Y, X);
            const int iy = min(max(pos.iy, 0), Hi - 2), ix = min(max(pos.ix, 0), Wi - 2);
            const uint8_t *q = img2 + (size_t)iy * stride2 + ix;
            const uint32_t lo = lsa_ld2(q), hi = lsa_ld2(q + stride2);
            const double P = ((pos.w[0] * (double)(lo & 0xffu) + pos.w[1] * (double)(lo >> 8)) +
                              pos.w[2] * (double)(hi & 0xffu)) +
                             pos.w[3] * (double)(hi >> 8);
            Sp = Sp + P;
            Spp = Spp + P * P;
            Sap = Sap + (double)aC * P;
            const int aR = row[u + 1];
            if (GRAD) {
                const int gx = aR - aL, gy = (int)row[u + tw] - (int)row[u - tw];
                const double phi[6] = {(double)gx, (double)(gx * u), (double)(gx * v),
                                       (double)gy, (double)(gy * u), (double)(gy * v)};
#pragma unroll
                for (int k = 0; k < 6; ++k) T[k] = T[k] + phi[k] * P;
            }
            aL = aC, aC = aR;
        }
    }
}

// grid: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells
__global__ __launch_bounds__(PHO_TX *PHO_TY) void k_lsm_affine(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                              size_t stride2, int Hi, int Wi, const double *d_row,
                                                              const double *d_col, int H, int W, int tiles_x, int oy,
                                                              int ox, int r, int iters, double max_move,
                                                              double max_shear, const uint8_t *mask, double *out_row,
                                                              double *out_col, double *score, int8_t *status,
                                                              double *affine)
{
    __shared__ uint8_t tile[LSA_TH * LSA_TW];
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int tw = PHO_TX + 2 * (r + 1), th = PHO_TY + 2 * (r + 1);
    {      // the img1 tile with its halo: tile[i][j] = img1[y0 + i][x0 + j], 0 outside the image
        const int64_t y0 = (int64_t)tile_y * PHO_TY + oy - (r + 1), x0 = (int64_t)tile_x * PHO_TX + ox - (r + 1);
        for (int i = threadIdx.x; i < th * tw; i += PHO_TX * PHO_TY) {
            const int64_t gy = y0 + i / tw, gx = x0 + i % tw;
            tile[i] = (gy >= 0 && gy < Hi && gx >= 0 && gx < Wi) ? img1[(size_t)gy * stride1 + (size_t)gx] : (uint8_t)0;
        }
    }
    __syncthreads();
    int y, x;
    if (!pho_cell(tiles_x, H, W, y, x)) return;
    const size_t c = (size_t)y * W + x;
    const double dr = d_row[c], dc = d_col[c];
    const double NaN = dm_nan();
    double o_row = dr, o_col = dc, o_score = NaN, o_a = NaN, o_b = NaN, o_c = NaN, o_d = NaN;
    int o_status = 0;
    const int cy = y + oy, cx = x + ox;
    const bool live = (!mask || mask[c] != 0) && pho_finite(dr) && pho_finite(dc) && cy >= r + 1 && cy <= Hi - r - 2 &&
                      cx >= r + 1 && cx <= Wi - r - 2;
    if (live) {
        const uint8_t *t = tile + ((int)(threadIdx.x / PHO_TX) + r + 1) * tw + (int)(threadIdx.x % PHO_TX) + r + 1;
        LsaCell m;
        const double py0 = (double)cy - dr, px0 = (double)cx - dc;
        if (!lsa_moments_factor(t, tw, r, m)) {
            o_status = -1;
        } else if (!(py0 >= (double)r && py0 < (double)(Hi - r - 1) && px0 >= (double)r && px0 < (double)(Wi - r - 1))) {
            o_status = -2;
        } else {
            const double s0 = lsa_start(t, tw, img2, stride2, r, py0, px0, m);
            double p[6] = {px0, 0.0, 0.0, py0, 0.0, 0.0}, Sp, Spp, Sap, T[6];
            int st = lsa_warp_ok(p, r, Hi, Wi) ? iters : -2;
            for (int it = 1; it <= iters && st == iters; ++it) {
                lsa_sums<true>(t, tw, img2, stride2, Hi, Wi, r, p, Sp, Spp, Sap, T);
                const double num = m.n * Sap - m.sa * Sp, vb = m.n * Spp - Sp * Sp;
                if (!(vb > 0.0)) {
                    st = -1;
                    break;
                }
                const double alpha = num / vb;
                double z[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    z[i] = m.RA[i] - alpha * (m.n * T[i] - m.f[i] * Sp);
#pragma unroll
                    for (int k = 0; k < i; ++k) z[i] = z[i] - m.L[LSA_LOW(i, k)] * z[k];
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    z[i] = z[i] / m.d[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) z[i] = z[i] - m.L[LSA_LOW(k, i)] * z[k];
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) p[k] = p[k] + 2.0 * z[k];
                if (!(fabs(p[0] - px0) <= max_move && fabs(p[3] - py0) <= max_move && fabs(p[1]) <= max_shear &&
                      fabs(p[2]) <= max_shear && fabs(p[4]) <= max_shear && fabs(p[5]) <= max_shear &&
                      lsa_warp_ok(p, r, Hi, Wi)))
                    st = -2;
            }
            o_score = s0;
            if (st == iters) {
                lsa_sums<false>(t, tw, img2, stride2, Hi, Wi, r, p, Sp, Spp, Sap, T);
                const double num = m.n * Sap - m.sa * Sp, vb = m.n * Spp - Sp * Sp;
                const double s1 = pho_zncc(m.VA, num, vb);
                if (s1 > s0) {
                    o_row = (double)cy - p[3];
                    o_col = (double)cx - p[0];
                    o_score = s1;
                    o_a = p[1], o_b = p[2], o_c = p[4], o_d = p[5];
                } else {
                    st = -3;
                }
            }
            o_status = st;
        }
    }
    out_row[c] = o_row;
    out_col[c] = o_col;
    if (score) score[c] = o_score;
    if (status) status[c] = (int8_t)o_status;
    if (affine) {
        const size_t plane = (size_t)H * W;
        affine[c] = o_a;
        affine[plane + c] = o_b;
        affine[2 * plane + c] = o_c;
        affine[3 * plane + c] = o_d;
    }
}

// ---- host side ------------------------------------------------------------------------------
// false for a shape the entry does not take
static bool lsa_plan(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t iters)
{
    if (radius < LSA_RMIN || radius > PHO_RMAX || iters < 1 || iters > LSA_ITMAX) return false;
    return pho_pair_plan(Hi, Wi, H, W);
}

extern "C" {

size_t dm_lsm_affine_bytes(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t iters)
{
    return lsa_plan(Hi, Wi, H, W, radius, iters) ? 16 : 0;
}

int dm_lsm_affine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t Hi,
                  int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W, int32_t oy, int32_t ox,
                  int32_t radius, int32_t iters, double max_move, double max_shear, int32_t flags,
                  const uint8_t *d_mask, double *d_out_row, double *d_out_col, double *d_score, int8_t *d_status,
                  double *d_affine, void *d_work, void *stream)
{
    if (!d_img1 || !d_img2 || !d_row || !d_col || !d_out_row || !d_out_col || !d_work)
        return dm_fail(DM_ERR_ARG, "null image / disparity / output / workspace pointer");
    if (const int bad = pho_pair_args(stride1, stride2, Hi, Wi, H, W, oy, ox, radius)) return bad;
    if (radius < LSA_RMIN)
        return dm_fail(DM_ERR_ARG, "radius must be in [%d, %d] for the affine model (got %d)", LSA_RMIN, PHO_RMAX, radius);
    if (iters < 1 || iters > LSA_ITMAX) return dm_fail(DM_ERR_ARG, "iters must be in [1, %d] (got %d)", LSA_ITMAX, iters);
    if (!(max_move > 0.0 && max_move <= 2.0)) return dm_fail(DM_ERR_ARG, "max_move must be in (0, 2] (got %g)", max_move);
    if (!(max_shear > 0.0 && max_shear < 1.0)) return dm_fail(DM_ERR_ARG, "max_shear must be in (0, 1) (got %g)", max_shear);
    if (flags != 0) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    if (!lsa_plan(Hi, Wi, H, W, radius, iters))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "affine lsm of %d x %d cells on a %d x %d image (at most 2^31 - 1 cells, 2^30 pixels a side)", H, W,
                     Hi, Wi);
    int tiles_x;
    const dim3 grid = pho_grid(H, W, &tiles_x);
    k_lsm_affine<<<grid, PHO_TX * PHO_TY, 0, (hipStream_t)stream>>>(
        d_img1, (size_t)stride1, d_img2, (size_t)stride2, Hi, Wi, d_row, d_col, H, W, tiles_x, oy, ox, radius, iters,
        max_move, max_shear, d_mask, d_out_row, d_out_col, d_score, d_status, d_affine);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
