// dm_photo.hip -- gfx950 kernel + C ABI of the photo-consistency score of a disparity map
// (dm_photo_score, include/dmstereo.h): the zero-mean normalised cross-correlation of the
// (2r+1)^2 window of img1 around a cell with img2 resampled bilinearly at the position the map
// claims, from exact integer moments.
//
// With (fy, fx) the fractional part of the claimed position, the resampled window is
// w0 P0 + w1 P1 + w2 P2 + w3 P3, the four integer-shifted windows of img2 under the bilinear
// weights, so its covariance with the img1 window A and its variance are bilinear / quadratic
// forms in w of the integers
//   CA_k = n sum(A P_k) - sum(A) sum(P_k),  CB_kl = n sum(P_k P_l) - sum(P_k) sum(P_l),
//   VA = n sum(A^2) - sum(A)^2
// which the kernel accumulates exactly; only about fifty float64 operations follow, in the
// order the header fixes.  tests/test_photo_host.py restates the definition in plain loops
// (photo_restate); the kernel equals it bit for bit.
//
// k_photo<ND>: one launch, one thread per cell, workgroups of 32 x 8 cells.  A thread walks the
// 2r+2 rows of its img2 patch.  A row of 2r+2 bytes is read as ND = (r + 2) / 2 dwords from its
// own byte address (no alignment is assumed; the tail is read as the dword that ends with the
// row's last byte, so no byte outside the row is touched), and gives the two shifted rows L
// (bytes 0 .. 2r) and R (bytes 1 .. 2r+1), zero beyond 2r.  The row of the img1 window is read
// the same way.  Every sum of products is then a chain of v_dot4_u32_u8 (__builtin_amdgcn_udot4)
// over the ND dwords: per patch row L.1, R.1, L.L, R.R, L.R, against the row above L.L', R.R',
// L'.R, R'.L, and against the two img1 rows it meets a.L, a.R, a'.L, a'.R, plus a.1 and a.a.
// All twenty sums stay below 225 * 255^2 < 2^24 and are kept in 32-bit registers; the products
// with n and of two sums need more than 32 bits (n sum(P P) reaches 3.29e9 at r = 7) and are
// formed in int64.  Every result is below 2^53 in magnitude, so the conversion to double is
// exact.
//
// Both images are read from global memory.  The windows of neighbouring cells overlap in all but
// one column, and neighbouring cells have neighbouring disparities, so the rows come from the
// vector L1 / L2; a byte-packed LDS tile of img1 would have to be read at byte granularity
// (DESIGN.md 4j).  A cell reads only its own d_row / d_col and writes only its own cells of the
// outputs and of d_maps, so d_row and d_col may be planes of d_maps.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "dm_photo.h"

// grid: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells.  ND = (r + 2) / 2 dwords per row.
template <int ND>
__global__ __launch_bounds__(PHO_TX *PHO_TY) void k_photo(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                         size_t stride2, int Hi, int Wi, const double *d_row,
                                                         const double *d_col, int H, int W, int tiles_x, int oy,
                                                         int ox, int r, int reject, double min_score, double *maps,
                                                         int M, double *score, double *warped, uint8_t *rejected)
{
    int y, x;
    if (!pho_cell(tiles_x, H, W, y, x)) return;
    const size_t c = (size_t)y * W + x;
    const double dr = d_row[c], dc = d_col[c];
    double s = dm_nan(), wv = dm_nan();
    if (pho_finite(dr) && pho_finite(dc)) {
        const int cy = y + oy, cx = x + ox;
        const double py = (double)cy - dr, px = (double)cx - dc;
        // the tests on py and px are made in double: only a position inside the image is converted
        const bool in4 = py >= 0.0 && py < (double)(Hi - 1) && px >= 0.0 && px < (double)(Wi - 1);
        if (in4) {
            const PhoPos pos = pho_bilin(py, px);
            const int iy = pos.iy, ix = pos.ix;
            const double(&w)[4] = pos.w;
            if (warped) {
                const uint8_t *q = img2 + (size_t)iy * stride2 + ix;
                wv = ((w[0] * (double)q[0] + w[1] * (double)q[1]) + w[2] * (double)q[stride2]) +
                     w[3] * (double)q[stride2 + 1];
            }
            const bool win1 = cy >= r && cy <= Hi - 1 - r && cx >= r && cx <= Wi - 1 - r;
            const bool win2 = iy >= r && iy <= Hi - 2 - r && ix >= r && ix <= Wi - 2 - r;
            if (win1 && win2 && (score || reject)) {
                const int D = 2 * r + 1;
                uint32_t mask[ND];
                pho_wmask<ND>(D, mask);
                const uint8_t *pa = img1 + (size_t)(cy - r) * stride1 + (cx - r);
                const uint8_t *pb = img2 + (size_t)(iy - r) * stride2 + (ix - r);
                uint32_t sa = 0, saa = 0, S0 = 0, S1 = 0, S2 = 0, S3 = 0, A0 = 0, A1 = 0, A2 = 0, A3 = 0;
                uint32_t B00 = 0, B01 = 0, B02 = 0, B03 = 0, B11 = 0, B12 = 0, B13 = 0, B22 = 0, B23 = 0, B33 = 0;
                uint32_t Lp[ND], Rp[ND], ap[ND];      // the row above
#pragma unroll
                for (int k = 0; k < ND; ++k) Lp[k] = Rp[k] = ap[k] = 0;
                for (int q = 0; q <= D; ++q) {
                    uint32_t raw[ND], Lc[ND], Rc[ND], ac[ND];
                    pho_row<ND>(pb + (size_t)q * stride2, D + 1, raw);
#pragma unroll
                    for (int k = 0; k < ND; ++k) {
                        const uint32_t up = k + 1 < ND ? raw[k + 1 < ND ? k + 1 : k] : 0u;
                        Lc[k] = raw[k] & mask[k];
                        Rc[k] = ((raw[k] >> 8) | (up << 24)) & mask[k];
                    }
                    const uint32_t sL = pho_sum<ND>(Lc, 0), sR = pho_sum<ND>(Rc, 0);
                    const uint32_t LL = pho_dot<ND>(Lc, Lc, 0), RR = pho_dot<ND>(Rc, Rc, 0), LR = pho_dot<ND>(Lc, Rc, 0);
                    if (q < D) {      // a row of P0 and P1, and of the img1 window
                        S0 += sL, S1 += sR, B00 += LL, B11 += RR, B01 += LR;
                        pho_row<ND>(pa + (size_t)q * stride1, D, ac);
#pragma unroll
                        for (int k = 0; k < ND; ++k) ac[k] &= mask[k];
                        sa = pho_sum<ND>(ac, sa);
                        saa = pho_dot<ND>(ac, ac, saa);
                        A0 = pho_dot<ND>(ac, Lc, A0);
                        A1 = pho_dot<ND>(ac, Rc, A1);
                    }
                    if (q > 0) {      // a row of P2 and P3: it meets row q - 1 of P0, P1 and of the img1 window
                        S2 += sL, S3 += sR, B22 += LL, B33 += RR, B23 += LR;
                        A2 = pho_dot<ND>(ap, Lc, A2);
                        A3 = pho_dot<ND>(ap, Rc, A3);
                        B02 = pho_dot<ND>(Lp, Lc, B02);
                        B03 = pho_dot<ND>(Lp, Rc, B03);
                        B12 = pho_dot<ND>(Rp, Lc, B12);
                        B13 = pho_dot<ND>(Rp, Rc, B13);
                    }
#pragma unroll
                    for (int k = 0; k < ND; ++k) {
                        Lp[k] = Lc[k], Rp[k] = Rc[k];
                        if (q < D) ap[k] = ac[k];
                    }
                }
                const int64_t n = (int64_t)D * D, Sa = sa;
                const double VA = (double)(n * (int64_t)saa - Sa * Sa);
                const uint32_t S[4] = {S0, S1, S2, S3}, A[4] = {A0, A1, A2, A3};
                const uint32_t B[10] = {B00, B01, B02, B03, B11, B12, B13, B22, B23, B33};
                double num, vb;
                pho_numvb(n, Sa, w, S, A, B, num, vb);
                s = pho_zncc(VA, num, vb);
            }
        }
    }
    if (score) score[c] = s;
    if (warped) warped[c] = wv;
    if (reject) {
        const bool rej = s < min_score;      // (false for an unscored cell: its s is NaN)
        if (rejected) rejected[c] = rej ? 1 : 0;
        if (rej) {
            const size_t cells = (size_t)H * W;
            for (int m = 0; m < M; ++m) maps[(size_t)m * cells + c] = dm_nan();
        }
    }
}

// ---- host side ------------------------------------------------------------------------------
// false for a shape the entry does not take (the limits of dm_median_bytes)
static bool pho_plan(int32_t M, int32_t H, int32_t W) { return dm_maps_plan(M, H, W, 64 * 65535); }

extern "C" {

size_t dm_photo_bytes(int32_t M, int32_t H, int32_t W) { return pho_plan(M, H, W) ? 16 : 0; }

int dm_photo_score(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t Hi,
                   int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W, int32_t oy,
                   int32_t ox, int32_t radius, int32_t flags, double min_score, double *d_maps, int32_t M,
                   double *d_score, double *d_warped, uint8_t *d_rejected, void *d_work, void *stream)
{
    if (!d_img1 || !d_img2 || !d_row || !d_col || !d_work)
        return dm_fail(DM_ERR_ARG, "null image / disparity / workspace pointer");
    if (const int bad = pho_pair_args(stride1, stride2, Hi, Wi, H, W, oy, ox, radius)) return bad;
    if (flags & ~DM_PHOTO_REJECT) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    const int reject = (flags & DM_PHOTO_REJECT) ? 1 : 0;
    if (reject) {
        if (!d_maps) return dm_fail(DM_ERR_ARG, "DM_PHOTO_REJECT needs d_maps");
        if (M < 1) return dm_fail(DM_ERR_ARG, "bad map count M=%d", M);
        if (!(min_score >= -1.0 && min_score <= 1.0))
            return dm_fail(DM_ERR_ARG, "min_score must be in [-1, 1] (got %g)", min_score);
    } else {
        if (d_rejected) return dm_fail(DM_ERR_ARG, "d_rejected needs DM_PHOTO_REJECT");
        if (!d_score && !d_warped) return dm_fail(DM_ERR_ARG, "no output: d_score and d_warped are null");
        M = 1;      // (d_maps and M are not read)
    }
    if (!pho_plan(M, H, W))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "photo score of %d maps of %d x %d cells (at most 65535 maps of 2^31 - 1 cells)", M, H, W);
    int tiles_x;
    const dim3 grid = pho_grid(H, W, &tiles_x);
    hipStream_t st = (hipStream_t)stream;
#define PHO_GO(ND_)                                                                                              \
    k_photo<ND_><<<grid, PHO_TX * PHO_TY, 0, st>>>(d_img1, (size_t)stride1, d_img2, (size_t)stride2, Hi, Wi, d_row, \
                                                   d_col, H, W, tiles_x, oy, ox, radius, reject, min_score,        \
                                                   reject ? d_maps : nullptr, M, d_score, d_warped, d_rejected)
    PHO_SWITCH_ND(radius, PHO_GO)
#undef PHO_GO
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
