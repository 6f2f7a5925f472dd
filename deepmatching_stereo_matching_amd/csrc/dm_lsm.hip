// dm_lsm.hip -- gfx950 kernel + C ABI of the least-squares sub-pixel matching of a disparity map
// (dm_lsm_refine, include/dmstereo.h): every cell linearises img1 around its window (doubled
// central differences Gx, Gy), and in each of `iters` steps solves the 2 x 2 normal equations for
// the shift that best explains the window of img1 by img2 resampled at the current position, gain
// and offset left free.  The step is kept only if dm_photo_score's ZNCC rises.
//
// k_lsm<ND>: one launch, one thread per cell, workgroups of 32 x 8 cells.  All sums are exact
// integers, chains of v_dot4_u32_u8 over rows read as unaligned dwords (dm_photo.h).  A row of the
// img1 window with its halo, 2r+3 bytes, is read once and cut into the three shifted rows
// L (columns -1), C and R (columns +1); the rows above and below a tap are the C of the
// neighbouring image rows.  The signed gradient sums are differences of unsigned chains:
// sum(Gx P) = R.P - L.P, sum(Gy P) = C(below).P - C(above).P, sum(Gx^2) = R.R + L.L - 2 R.L, ...
//   once per cell   lsm_moments: one walk over the 2r+3 halo rows of img1, 20 chains a row
//   each step       lsm_walk<ND, true>: one walk over the 2r+2 rows of the img2 patch at the
//                   current integer position; a row meets the upper windows P0, P1 and the lower
//                   ones P2, P3, each against C, L, R and the C above and below: dm_photo_score's
//                   20 chains plus 16 gradient chains.  The img1 rows are read again from L1 and
//                   held in a rolling window of four image rows.
//   at the end      lsm_walk<ND, false>: the score of the final position (the score of the start
//                   is a by-product of the first step's walk), so a cell makes iters + 1 walks.
// Every chain stays below 225 * 255^2 < 2^24; the products with n and of two sums are int64 and
// below 2^53; the determinant is formed in double.  The float64 tail is the header's, operation
// for operation, under -ffp-contract=off.
//
// Reads: the img1 halo window lies inside the image by rule 1, tested before anything is read.  A
// position is tested in double (r <= p < side - r - 1) before it is converted, and the converted
// integer is tested again, so the 2r+2 rows and columns of the img2 patch lie inside the image;
// a row is read as exactly its 2r+2 (img2) or 2r+3 (img1) bytes.  A cell reads only its own
// d_row / d_col and does so before it writes, so the outputs may alias the inputs.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "dm_photo.h"

#define LSM_ITMAX 8

struct LsmSums {
    uint32_t S[4], A[4], B[10];                  // dm_photo_score's: sum P_k, sum(A P_k), sum(P_k P_l)
    uint32_t XR[4], XL[4], YD[4], YU[4];         // sum(A-> P_k), sum(A<- P_k), sum(A-below P_k), sum(A-above P_k)
};

struct LsmMoments {
    int64_t sa, gx, gy;
    double VA, Hxx, Hyy, Hxy, RAx, RAy, D;
};

// rule 2: pa is the top-left byte of the halo window, (cy-r-1, cx-r-1)
template <int ND>
__device__ __forceinline__ LsmMoments lsm_moments(const uint8_t *pa, size_t stride1, int D, const uint32_t (&wm)[ND])
{
    uint32_t sa = 0, saa = 0, sR = 0, sL = 0, sD = 0, sU = 0, RR = 0, LL = 0, RL = 0, DD = 0, UU = 0, DU = 0;
    uint32_t RD = 0, RU = 0, LD = 0, LU = 0, RC = 0, LC = 0, DC = 0, UC = 0;
    uint32_t Cp[ND], Lp[ND], Rp[ND], Cpp[ND];      // the row above, and the C two rows above
#pragma unroll
    for (int k = 0; k < ND; ++k) Cp[k] = Lp[k] = Rp[k] = Cpp[k] = 0;
    for (int q = 0; q <= D + 1; ++q) {      // halo row q is window row q - 1
        uint32_t raw[ND + 1], Lc[ND], Cc[ND], Rc[ND];
        pho_rowz<ND + 1>(pa + (size_t)q * stride1, D + 2, raw);
        pho_shift<0>(raw, wm, Lc);
        pho_shift<1>(raw, wm, Cc);
        pho_shift<2>(raw, wm, Rc);
        const uint32_t sC = pho_sum<ND>(Cc, 0), CC = pho_dot<ND>(Cc, Cc, 0), CCp = pho_dot<ND>(Cc, Cp, 0);
        if (q >= 1 && q <= D) {      // a row of the window: the taps, their left and right neighbours
            sa += sC, saa += CC;
            sR = pho_sum<ND>(Rc, sR);
            sL = pho_sum<ND>(Lc, sL);
            RR = pho_dot<ND>(Rc, Rc, RR);
            LL = pho_dot<ND>(Lc, Lc, LL);
            RL = pho_dot<ND>(Rc, Lc, RL);
            RC = pho_dot<ND>(Rc, Cc, RC);
            LC = pho_dot<ND>(Lc, Cc, LC);
            UC += CCp;                          // the row above this window row
            RU = pho_dot<ND>(Rc, Cp, RU);
            LU = pho_dot<ND>(Lc, Cp, LU);
        }
        if (q <= D - 1) sU += sC, UU += CC;     // the row above window row q
        if (q >= 2) {                           // the row below window row q - 2
            sD += sC, DD += CC;
            DC += CCp;
            DU = pho_dot<ND>(Cc, Cpp, DU);
            RD = pho_dot<ND>(Cc, Rp, RD);
            LD = pho_dot<ND>(Cc, Lp, LD);
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) Cpp[k] = Cp[k], Cp[k] = Cc[k], Lp[k] = Lc[k], Rp[k] = Rc[k];
    }
    const int64_t n = (int64_t)D * D;
    LsmMoments m;
    m.sa = sa;
    m.gx = (int64_t)sR - (int64_t)sL;
    m.gy = (int64_t)sD - (int64_t)sU;
    const int64_t Gxx = (int64_t)RR + (int64_t)LL - 2 * (int64_t)RL, Gyy = (int64_t)DD + (int64_t)UU - 2 * (int64_t)DU;
    const int64_t Gxy = ((int64_t)RD - (int64_t)RU) - ((int64_t)LD - (int64_t)LU);
    const int64_t GxA = (int64_t)RC - (int64_t)LC, GyA = (int64_t)DC - (int64_t)UC;
    m.VA = (double)(n * (int64_t)saa - m.sa * m.sa);
    m.Hxx = (double)(n * Gxx - m.gx * m.gx);
    m.Hyy = (double)(n * Gyy - m.gy * m.gy);
    m.Hxy = (double)(n * Gxy - m.gx * m.gy);
    m.RAx = (double)(n * GxA - m.gx * m.sa);
    m.RAy = (double)(n * GyA - m.gy * m.sa);
    m.D = m.Hxx * m.Hyy - m.Hxy * m.Hxy;
    return m;
}

// the sums of one position: pa as in lsm_moments, pb the top-left byte of the img2 patch, (iy-r, ix-r).
// Patch row q is row q of the upper windows P0, P1 (q < D) and row q - 1 of the lower ones P2, P3 (q > 0);
// window row u has its taps in halo row u + 1, the rows above and below them in halo rows u and u + 2.
template <int ND, bool GRAD>
__device__ __forceinline__ void lsm_walk(const uint8_t *pa, size_t stride1, const uint8_t *pb, size_t stride2, int D,
                                         const uint32_t (&wm)[ND], LsmSums &s)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) s.S[k] = s.A[k] = s.XR[k] = s.XL[k] = s.YD[k] = s.YU[k] = 0;
#pragma unroll
    for (int k = 0; k < 10; ++k) s.B[k] = 0;
    // halo rows q - 1 (Cm), q (L0 C0 R0) and q + 1 (L1 C1 R1) of img1, and patch row q - 1 (Lp Rp)
    uint32_t Cm[ND], L0[ND], C0[ND], R0[ND], L1[ND], C1[ND], R1[ND], Lp[ND], Rp[ND];
    {
        uint32_t raw[ND + 1];
        pho_rowz<ND + 1>(pa, D + 2, raw);
        pho_shift<1>(raw, wm, C0);
        pho_rowz<ND + 1>(pa + stride1, D + 2, raw);
        pho_shift<0>(raw, wm, L1);
        pho_shift<1>(raw, wm, C1);
        pho_shift<2>(raw, wm, R1);
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) Cm[k] = L0[k] = R0[k] = Lp[k] = Rp[k] = 0;
    for (int q = 0; q <= D; ++q) {
        uint32_t rawb[ND], Lc[ND], Rc[ND], L2[ND], C2[ND], R2[ND];
        pho_row<ND>(pb + (size_t)q * stride2, D + 1, rawb);
        pho_shift<0>(rawb, wm, Lc);
        pho_shift<1>(rawb, wm, Rc);
        const uint32_t sL = pho_sum<ND>(Lc, 0), sR = pho_sum<ND>(Rc, 0);
        const uint32_t LL = pho_dot<ND>(Lc, Lc, 0), RR = pho_dot<ND>(Rc, Rc, 0), LR = pho_dot<ND>(Lc, Rc, 0);
#pragma unroll
        for (int k = 0; k < ND; ++k) L2[k] = C2[k] = R2[k] = 0;
        if (q < D) {      // a row of P0 and P1: window row q
            uint32_t raw[ND + 1];
            pho_rowz<ND + 1>(pa + (size_t)(q + 2) * stride1, D + 2, raw);
            pho_shift<0>(raw, wm, L2);
            pho_shift<1>(raw, wm, C2);
            pho_shift<2>(raw, wm, R2);
            s.S[0] += sL, s.S[1] += sR, s.B[0] += LL, s.B[4] += RR, s.B[1] += LR;
            s.A[0] = pho_dot<ND>(C1, Lc, s.A[0]);
            s.A[1] = pho_dot<ND>(C1, Rc, s.A[1]);
            if (GRAD) {
                s.XR[0] = pho_dot<ND>(R1, Lc, s.XR[0]);
                s.XR[1] = pho_dot<ND>(R1, Rc, s.XR[1]);
                s.XL[0] = pho_dot<ND>(L1, Lc, s.XL[0]);
                s.XL[1] = pho_dot<ND>(L1, Rc, s.XL[1]);
                s.YD[0] = pho_dot<ND>(C2, Lc, s.YD[0]);
                s.YD[1] = pho_dot<ND>(C2, Rc, s.YD[1]);
                s.YU[0] = pho_dot<ND>(C0, Lc, s.YU[0]);
                s.YU[1] = pho_dot<ND>(C0, Rc, s.YU[1]);
            }
        }
        if (q > 0) {      // a row of P2 and P3: window row q - 1; it meets row q - 1 of P0 and P1
            s.S[2] += sL, s.S[3] += sR, s.B[7] += LL, s.B[9] += RR, s.B[8] += LR;
            s.A[2] = pho_dot<ND>(C0, Lc, s.A[2]);
            s.A[3] = pho_dot<ND>(C0, Rc, s.A[3]);
            s.B[2] = pho_dot<ND>(Lp, Lc, s.B[2]);
            s.B[3] = pho_dot<ND>(Lp, Rc, s.B[3]);
            s.B[5] = pho_dot<ND>(Rp, Lc, s.B[5]);
            s.B[6] = pho_dot<ND>(Rp, Rc, s.B[6]);
            if (GRAD) {
                s.XR[2] = pho_dot<ND>(R0, Lc, s.XR[2]);
                s.XR[3] = pho_dot<ND>(R0, Rc, s.XR[3]);
                s.XL[2] = pho_dot<ND>(L0, Lc, s.XL[2]);
                s.XL[3] = pho_dot<ND>(L0, Rc, s.XL[3]);
                s.YD[2] = pho_dot<ND>(C1, Lc, s.YD[2]);
                s.YD[3] = pho_dot<ND>(C1, Rc, s.YD[3]);
                s.YU[2] = pho_dot<ND>(Cm, Lc, s.YU[2]);
                s.YU[3] = pho_dot<ND>(Cm, Rc, s.YU[3]);
            }
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            Cm[k] = C0[k], L0[k] = L1[k], C0[k] = C1[k], R0[k] = R1[k];
            L1[k] = L2[k], C1[k] = C2[k], R1[k] = R2[k];
            Lp[k] = Lc[k], Rp[k] = Rc[k];
        }
    }
}

// rule 3 of dm_photo_score on a position, in double: NaN fails
__device__ __forceinline__ bool lsm_inside(double py, double px, int Hi, int Wi, int r)
{
    return py >= (double)r && py < (double)(Hi - r - 1) && px >= (double)r && px < (double)(Wi - r - 1);
}

// a position that passed lsm_inside -> the patch's corner, the bilinear weights; false if the integer test fails
// (it cannot: the test repeats lsm_inside on the converted value, before anything is read)
__device__ __forceinline__ bool lsm_split(double py, double px, int Hi, int Wi, int r, int &iy, int &ix, double (&w)[4])
{
    const PhoPos pos = pho_bilin(py, px);
    iy = pos.iy, ix = pos.ix;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = pos.w[k];
    return iy >= r && iy <= Hi - r - 2 && ix >= r && ix <= Wi - r - 2;
}

// grid: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells.  ND = (r + 2) / 2 dwords per window row.
template <int ND>
__global__ __launch_bounds__(PHO_TX *PHO_TY) void k_lsm(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                       size_t stride2, int Hi, int Wi, const double *d_row,
                                                       const double *d_col, int H, int W, int tiles_x, int oy, int ox,
                                                       int r, int iters, double max_move, const uint8_t *mask,
                                                       double *out_row, double *out_col, double *score, int8_t *status)
{
    int y, x;
    if (!pho_cell(tiles_x, H, W, y, x)) return;
    const size_t c = (size_t)y * W + x;
    const double dr = d_row[c], dc = d_col[c];
    const double NaN = dm_nan();
    double o_row = dr, o_col = dc, o_score = NaN;
    int o_status = 0;
    const int cy = y + oy, cx = x + ox;
    const bool live = (!mask || mask[c] != 0) && pho_finite(dr) && pho_finite(dc) && cy >= r + 1 && cy <= Hi - r - 2 &&
                      cx >= r + 1 && cx <= Wi - r - 2;
    if (live) {
        const int D = 2 * r + 1;
        const int64_t n = (int64_t)D * D;
        uint32_t wm[ND];
        pho_wmask<ND>(D, wm);
        const uint8_t *pa = img1 + (size_t)(cy - r - 1) * stride1 + (cx - r - 1);
        const LsmMoments m = lsm_moments<ND>(pa, stride1, D, wm);
        const double py0 = (double)cy - dr, px0 = (double)cx - dc;
        if (!(m.D > 0.0)) {
            o_status = -1;
        } else if (!lsm_inside(py0, px0, Hi, Wi, r)) {
            o_status = -2;
        } else {
            double py = py0, px = px0, s0 = NaN, w[4], num, vb;
            int iy, ix, st = iters;
            LsmSums s;
            for (int t = 1; t <= iters; ++t) {
                if (!lsm_split(py, px, Hi, Wi, r, iy, ix, w)) {
                    st = -2;
                    break;
                }
                lsm_walk<ND, true>(pa, stride1, img2 + (size_t)(iy - r) * stride2 + (ix - r), stride2, D, wm, s);
                pho_numvb(n, m.sa, w, s.S, s.A, s.B, num, vb);
                if (t == 1) s0 = pho_zncc(m.VA, num, vb);
                if (!(vb > 0.0)) {
                    st = -1;
                    break;
                }
                double GX[4], GY[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    GX[k] = (double)(n * ((int64_t)s.XR[k] - (int64_t)s.XL[k]) - m.gx * (int64_t)s.S[k]);
                    GY[k] = (double)(n * ((int64_t)s.YD[k] - (int64_t)s.YU[k]) - m.gy * (int64_t)s.S[k]);
                }
                const double gbx = ((w[0] * GX[0] + w[1] * GX[1]) + w[2] * GX[2]) + w[3] * GX[3];
                const double gby = ((w[0] * GY[0] + w[1] * GY[1]) + w[2] * GY[2]) + w[3] * GY[3];
                const double alpha = num / vb;
                const double bx = m.RAx - alpha * gbx, by = m.RAy - alpha * gby;
                const double ux = ((m.Hyy * bx) - (m.Hxy * by)) / m.D, uy = ((m.Hxx * by) - (m.Hxy * bx)) / m.D;
                px = px + 2.0 * ux;
                py = py + 2.0 * uy;
                if (!(fabs(py - py0) <= max_move && fabs(px - px0) <= max_move && lsm_inside(py, px, Hi, Wi, r))) {
                    st = -2;
                    break;
                }
            }
            o_score = s0;
            if (st == iters && !lsm_split(py, px, Hi, Wi, r, iy, ix, w)) st = -2;
            if (st == iters) {
                lsm_walk<ND, false>(pa, stride1, img2 + (size_t)(iy - r) * stride2 + (ix - r), stride2, D, wm, s);
                pho_numvb(n, m.sa, w, s.S, s.A, s.B, num, vb);
                const double s1 = pho_zncc(m.VA, num, vb);
                if (s1 > s0) {
                    o_row = (double)cy - py;
                    o_col = (double)cx - px;
                    o_score = s1;
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
}

// ---- host side ------------------------------------------------------------------------------
// false for a shape the entry does not take
static bool lsm_plan(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t iters)
{
    if (radius < 1 || radius > PHO_RMAX || iters < 1 || iters > LSM_ITMAX) return false;
    return pho_pair_plan(Hi, Wi, H, W);
}

extern "C" {

size_t dm_lsm_refine_bytes(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t iters)
{
    return lsm_plan(Hi, Wi, H, W, radius, iters) ? 16 : 0;
}

int dm_lsm_refine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t Hi,
                  int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W, int32_t oy, int32_t ox,
                  int32_t radius, int32_t iters, double max_move, int32_t flags, const uint8_t *d_mask,
                  double *d_out_row, double *d_out_col, double *d_score, int8_t *d_status, void *d_work, void *stream)
{
    if (!d_img1 || !d_img2 || !d_row || !d_col || !d_out_row || !d_out_col || !d_work)
        return dm_fail(DM_ERR_ARG, "null image / disparity / output / workspace pointer");
    if (const int bad = pho_pair_args(stride1, stride2, Hi, Wi, H, W, oy, ox, radius)) return bad;
    if (iters < 1 || iters > LSM_ITMAX) return dm_fail(DM_ERR_ARG, "iters must be in [1, %d] (got %d)", LSM_ITMAX, iters);
    if (!(max_move > 0.0 && max_move <= 2.0)) return dm_fail(DM_ERR_ARG, "max_move must be in (0, 2] (got %g)", max_move);
    if (flags != 0) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    if (!lsm_plan(Hi, Wi, H, W, radius, iters))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "lsm refine of %d x %d cells on a %d x %d image (at most 2^31 - 1 cells, 2^30 pixels a side)", H, W,
                     Hi, Wi);
    int tiles_x;
    const dim3 grid = pho_grid(H, W, &tiles_x);
    hipStream_t st = (hipStream_t)stream;
#define LSM_GO(ND_)                                                                                             \
    k_lsm<ND_><<<grid, PHO_TX * PHO_TY, 0, st>>>(d_img1, (size_t)stride1, d_img2, (size_t)stride2, Hi, Wi, d_row,  \
                                                 d_col, H, W, tiles_x, oy, ox, radius, iters, max_move, d_mask,   \
                                                 d_out_row, d_out_col, d_score, d_status)
    PHO_SWITCH_ND(radius, LSM_GO)
#undef LSM_GO
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
