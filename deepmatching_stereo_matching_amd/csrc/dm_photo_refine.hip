// dm_photo_refine.hip -- gfx950 kernel + C ABI of the local re-matching of a disparity map
// (dm_photo_refine, include/dmstereo.h): every cell scores the (2s+1)^2 integer neighbours of the
// position its disparity claims with dm_photo_score's ZNCC and moves to the best one, optionally
// with a parabola through the winner's neighbours per axis.
//
// k_refine<ND, S>: one launch, one thread per cell, workgroups of 32 x 8 cells.  A candidate
// (dy, dx) needs the four img2 windows Q[dy + {0,1}][dx + {0,1}]; the candidates of one row dy
// share the two rows of windows Q[dy][.] and Q[dy + 1][.], K = 2S + 2 column shifts each.  So a
// thread makes one walk per candidate row: the 2r+2 image rows iy+dy-r .. iy+dy+r+1, each read
// once as unaligned dwords (dm_photo.h) from the first column any scored candidate needs to the
// last, and cut into the K shifted rows W[0 .. K) by funnel shifts.  Per image row and shift the
// walk adds, as chains of v_dot4_u32_u8, W.1, W.W, W[j].W[j+1] and a.W for the upper and for the
// lower window, and against the row above P[j].W[j], P[j].W[j+1], P[j+1].W[j]: 9 K - 4 chains
// where 2S+1 separate dm_photo_score walks make 20 (2S+1).  The twenty sums of candidate j of the
// row are then a selection of these, and the float64 tail is dm_photo_score's, operation for
// operation, so candidate (0, 0) has that entry's bits.  sum A and sum A^2 are taken once.
//
// Every sum stays below 225 * 255^2 < 2^24; the products with n and of two sums are int64.  The
// candidate rows and columns are clamped to the scored ones before anything is read, so no byte
// outside the image rows is touched: the first column read is ix+dxlo-r >= 0, the last
// ix+dxhi+r+1 <= Wi-1, and the tail dword ends with the last byte (at least 4 bytes are read:
// 2r+2 >= 4).  The (2S+1)^2 scores of a cell live in a per-thread array; the winner is found by
// one ordered scan, so the result does not depend on anything but the cell.  A cell reads only
// its own d_row / d_col and does so before it writes, so the outputs may alias the inputs.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "dm_photo.h"

#define REF_SMAX 3
#define REF_POSMAX 1073741824.0      // 2^30

// the parabola through (-1, sm), (0, s0), (1, sp): its peak, clamped to [-0.5, 0.5]; 0 unless it opens downwards
__device__ __forceinline__ double ref_peak(double sm, double s0, double sp)
{
    const double den = (sm + sp) - 2.0 * s0;
    if (!(den < 0.0)) return 0.0;
    const double t = (0.5 * (sm - sp)) / den;
    return t > 0.5 ? 0.5 : (t < -0.5 ? -0.5 : t);
}

// grid: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells.  ND = (r + 2) / 2 dwords per window row,
// S the search radius.
template <int ND, int S>
__global__ __launch_bounds__(PHO_TX *PHO_TY) void k_refine(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                          size_t stride2, int Hi, int Wi, const double *d_row,
                                                          const double *d_col, int H, int W, int tiles_x, int oy,
                                                          int ox, int r, double min_gain, int subpix,
                                                          const uint8_t *mask, double *out_row, double *out_col,
                                                          double *score, int8_t *shift)
{
    constexpr int NC = 2 * S + 1;                  // candidates a side
    constexpr int K = 2 * S + 2;                   // window shifts a side
    constexpr int NW = ND + (2 * S + 3) / 4;       // dwords of the widest row read: 4 ND + 2 S bytes
    int y, x;
    if (!pho_cell(tiles_x, H, W, y, x)) return;
    const size_t c = (size_t)y * W + x;
    const double dr = d_row[c], dc = d_col[c];
    const double NaN = dm_nan();
    double o_row = dr, o_col = dc, o_score = NaN;
    int o_dy = 0, o_dx = 0;
    const int cy = y + oy, cx = x + ox;
    bool live = (!mask || mask[c] != 0) && pho_finite(dr) && pho_finite(dc) && cy >= r && cy <= Hi - 1 - r &&
                cx >= r && cx <= Wi - 1 - r;
    double py = 0.0, px = 0.0;
    if (live) {
        py = (double)cy - dr, px = (double)cx - dc;
        // the test is made in double: only a position it passed is converted
        live = py >= -REF_POSMAX && py <= REF_POSMAX && px >= -REF_POSMAX && px <= REF_POSMAX;
    }
    if (live) {
        const PhoPos pos = pho_bilin(py, px);
        const int iy = pos.iy, ix = pos.ix;      // |iy|, |ix| <= 2^30
        const double(&w)[4] = pos.w;
        // the scored candidates: r <= iy + dy <= Hi - r - 2, r <= ix + dx <= Wi - r - 2 (no overflow: Hi, Wi <= 2^30)
        const int dylo = max(-S, r - iy), dyhi = min(S, Hi - r - 2 - iy);
        const int dxlo = max(-S, r - ix), dxhi = min(S, Wi - r - 2 - ix);
        double sc[NC * NC];
#pragma unroll
        for (int k = 0; k < NC * NC; ++k) sc[k] = NaN;
        if (dylo <= dyhi && dxlo <= dxhi) {
            const int D = 2 * r + 1;
            const int64_t n = (int64_t)D * D;
            const int ncand = dxhi - dxlo + 1;           // candidates of a row: 1 .. NC
            const int nbytes = ncand + D;                // bytes of an image row that they need: >= 4
            uint32_t wmask[ND], sa, saa;
            pho_wmask<ND>(D, wmask);
            const uint8_t *pa = img1 + (size_t)(cy - r) * stride1 + (cx - r);
            pho_moments1<ND>(pa, stride1, D, wmask, sa, saa);
            const int64_t Sa = sa;
            const double VA = (double)(n * (int64_t)saa - Sa * Sa);
            for (int dy = dylo; dy <= dyhi; ++dy) {
                const uint8_t *pb = img2 + (size_t)(iy + dy - r) * stride2 + (ix + dxlo - r);
                uint32_t St[K], Sb[K], Qt[K], Qb[K], At[K], Ab[K], Dn[K];      // per window: sums, squares, a., the window below
                uint32_t Et[K - 1], Eb[K - 1], Ds[K - 1], Dw[K - 1];           // per pair: ->, -> below, down-right, down-left
                uint32_t Pw[K][ND], ap[ND];                                    // the row above
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    St[j] = Sb[j] = Qt[j] = Qb[j] = At[j] = Ab[j] = Dn[j] = 0;
#pragma unroll
                    for (int k = 0; k < ND; ++k) Pw[j][k] = 0;
                }
#pragma unroll
                for (int j = 0; j < K - 1; ++j) Et[j] = Eb[j] = Ds[j] = Dw[j] = 0;
#pragma unroll
                for (int k = 0; k < ND; ++k) ap[k] = 0;
                for (int q = 0; q <= D; ++q) {
                    uint32_t raw[NW], Wc[K][ND], ac[ND];
                    pho_rowz<NW>(pb + (size_t)q * stride2, nbytes, raw);
#pragma unroll
                    for (int j = 0; j < K; ++j) {
#pragma unroll
                        for (int k = 0; k < ND; ++k) {
                            const int b = j + 4 * k, qd = b >> 2, rm = b & 3;      // compile-time after unrolling
                            const uint32_t lo = qd < NW ? raw[qd < NW ? qd : 0] : 0u;
                            const uint32_t hi = qd + 1 < NW ? raw[qd + 1 < NW ? qd + 1 : 0] : 0u;
                            const uint32_t v = rm ? ((lo >> (8 * rm)) | (hi << (32 - 8 * rm))) : lo;
                            Wc[j][k] = v & wmask[k];
                        }
                    }
                    if (q < D) {      // a row of the upper windows, and of the img1 window
                        pho_row<ND>(pa + (size_t)q * stride1, D, ac);
#pragma unroll
                        for (int k = 0; k < ND; ++k) ac[k] &= wmask[k];
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            St[j] = pho_sum<ND>(Wc[j], St[j]);
                            Qt[j] = pho_dot<ND>(Wc[j], Wc[j], Qt[j]);
                            At[j] = pho_dot<ND>(ac, Wc[j], At[j]);
                        }
#pragma unroll
                        for (int j = 0; j < K - 1; ++j) Et[j] = pho_dot<ND>(Wc[j], Wc[j + 1], Et[j]);
                    }
                    if (q > 0) {      // a row of the lower windows: it meets row q - 1 of the upper ones and of the img1 window
#pragma unroll
                        for (int j = 0; j < K; ++j) {
                            Sb[j] = pho_sum<ND>(Wc[j], Sb[j]);
                            Qb[j] = pho_dot<ND>(Wc[j], Wc[j], Qb[j]);
                            Ab[j] = pho_dot<ND>(ap, Wc[j], Ab[j]);
                            Dn[j] = pho_dot<ND>(Pw[j], Wc[j], Dn[j]);
                        }
#pragma unroll
                        for (int j = 0; j < K - 1; ++j) {
                            Eb[j] = pho_dot<ND>(Wc[j], Wc[j + 1], Eb[j]);
                            Ds[j] = pho_dot<ND>(Pw[j], Wc[j + 1], Ds[j]);
                            Dw[j] = pho_dot<ND>(Pw[j + 1], Wc[j], Dw[j]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < K; ++j)
#pragma unroll
                        for (int k = 0; k < ND; ++k) Pw[j][k] = Wc[j][k];
                    if (q < D) {
#pragma unroll
                        for (int k = 0; k < ND; ++k) ap[k] = ac[k];
                    }
                }
                // candidate j of this row: P0 = upper j, P1 = upper j+1, P2 = lower j, P3 = lower j+1
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    if (j < ncand) {
                        const uint32_t Sj[4] = {St[j], St[j + 1], Sb[j], Sb[j + 1]};
                        const uint32_t Aj[4] = {At[j], At[j + 1], Ab[j], Ab[j + 1]};
                        const uint32_t Bj[10] = {Qt[j], Et[j], Dn[j], Ds[j], Qt[j + 1], Dw[j], Dn[j + 1], Qb[j], Eb[j], Qb[j + 1]};
                        double num, vb;
                        pho_numvb(n, Sa, w, Sj, Aj, Bj, num, vb);      // dm_photo_score's rule 5, operation for operation
                        sc[(dy + S) * NC + (dxlo + S + j)] = pho_zncc(VA, num, vb);
                    }
                }
            }
            // the winner: the highest score; ties to the smallest dy^2 + dx^2, then the smaller dy, then the smaller dx
            // (the scan runs dy, then dx upwards, so among equal scores and distances the first one met stays)
            double best = NaN;
            int bdy = 0, bdx = 0, bd2 = 0;
            bool any = false;
            for (int k = 0; k < NC * NC; ++k) {
                const double s = sc[k];
                if (s != s) continue;
                const int dy = k / NC - S, dx = k % NC - S, d2 = dy * dy + dx * dx;
                if (!any || s > best || (s == best && d2 < bd2)) best = s, bdy = dy, bdx = dx, bd2 = d2, any = true;
            }
            if (any) {
                const double centre = sc[S * NC + S];
                if (centre == centre && !(best > centre + min_gain)) best = centre, bdy = 0, bdx = 0;
                o_score = best, o_dy = bdy, o_dx = bdx;
                if (bdy != 0 || bdx != 0) {
                    double ty = 0.0, tx = 0.0;
                    if (subpix) {
                        const int k = (bdy + S) * NC + (bdx + S);
                        if (bdy > -S && bdy < S) {
                            const double sm = sc[k - NC], sp = sc[k + NC];
                            if (sm == sm && sp == sp) ty = ref_peak(sm, best, sp);
                        }
                        if (bdx > -S && bdx < S) {
                            const double sm = sc[k - 1], sp = sc[k + 1];
                            if (sm == sm && sp == sp) tx = ref_peak(sm, best, sp);
                        }
                    }
                    o_row = dr - ((double)bdy + ty);
                    o_col = dc - ((double)bdx + tx);
                }
            }
        }
    }
    out_row[c] = o_row;
    out_col[c] = o_col;
    if (score) score[c] = o_score;
    if (shift) {
        shift[c] = (int8_t)o_dy;
        shift[(size_t)H * W + c] = (int8_t)o_dx;
    }
}

// ---- host side ------------------------------------------------------------------------------
// false for a shape the entry does not take
static bool ref_plan(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t search)
{
    if (radius < 1 || radius > PHO_RMAX || search < 1 || search > REF_SMAX) return false;
    return pho_pair_plan(Hi, Wi, H, W);
}

extern "C" {

size_t dm_photo_refine_bytes(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t search)
{
    return ref_plan(Hi, Wi, H, W, radius, search) ? 16 : 0;
}

int dm_photo_refine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t Hi,
                    int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W, int32_t oy, int32_t ox,
                    int32_t radius, int32_t search, double min_gain, int32_t flags, const uint8_t *d_mask,
                    double *d_out_row, double *d_out_col, double *d_score, int8_t *d_shift, void *d_work, void *stream)
{
    if (!d_img1 || !d_img2 || !d_row || !d_col || !d_out_row || !d_out_col || !d_work)
        return dm_fail(DM_ERR_ARG, "null image / disparity / output / workspace pointer");
    if (const int bad = pho_pair_args(stride1, stride2, Hi, Wi, H, W, oy, ox, radius)) return bad;
    if (search < 1 || search > REF_SMAX) return dm_fail(DM_ERR_ARG, "search must be in [1, %d] (got %d)", REF_SMAX, search);
    if (!(min_gain >= 0.0 && min_gain <= 2.0)) return dm_fail(DM_ERR_ARG, "min_gain must be in [0, 2] (got %g)", min_gain);
    if (flags & ~DM_REFINE_SUBPIX) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    if (!ref_plan(Hi, Wi, H, W, radius, search))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "photo refine of %d x %d cells on a %d x %d image (at most 2^31 - 1 cells, 2^30 pixels a side)", H,
                     W, Hi, Wi);
    int tiles_x;
    const dim3 grid = pho_grid(H, W, &tiles_x);
    hipStream_t st = (hipStream_t)stream;
    const int subpix = (flags & DM_REFINE_SUBPIX) ? 1 : 0;
#define REF_GO(ND_, S_)                                                                                               \
    k_refine<ND_, S_><<<grid, PHO_TX * PHO_TY, 0, st>>>(d_img1, (size_t)stride1, d_img2, (size_t)stride2, Hi, Wi, d_row, \
                                                        d_col, H, W, tiles_x, oy, ox, radius, min_gain, subpix, d_mask, \
                                                        d_out_row, d_out_col, d_score, d_shift)
#define REF_GO_S(ND_)                                                                                                 \
    switch (search) {                                                                                                 \
    case 1: REF_GO(ND_, 1); break;                                                                                    \
    case 2: REF_GO(ND_, 2); break;                                                                                    \
    default: REF_GO(ND_, 3); break;                                                                                   \
    }
    PHO_SWITCH_ND(radius, REF_GO_S)
#undef REF_GO_S
#undef REF_GO
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
