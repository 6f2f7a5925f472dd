/* dmstereo_lsm.h -- affine least-squares matching of a disparity map (csrc/dm_lsm_affine.hip).
 *
 * A third public header of libdmstereo.so, beside dmstereo.h, whose status codes it uses;
 * dm_abi_version() does not change with it.
 *
 * Not in the reference.  dm_lsm_refine (dmstereo.h) is least-squares matching (Gruen 1985) cut down
 * to a shift: it assumes that the img1 window looks the same in img2 apart from gain and offset,
 * which holds only where the disparity is constant across the window.  On a slope the matched
 * window is stretched or sheared, the shift-only solve is biased and its score falls.
 * dm_lsm_affine solves for the six geometric parameters of Gruen's method: the window of img1
 * around (cy, cx) is matched by img2 sampled at
 *     X(u, v) = px + ((1 + a) u + b v),    Y(u, v) = py + (c u + (1 + d) v)
 * for the tap with column offset u and row offset v, both in [-r, r].  1 + a is dx2/dx1: -a and -d
 * are the disparity gradients along the columns and along the rows.
 *
 * Inputs.  Images, planes d_row / d_col, offsets oy, ox, iters in [1, 8] and max_move in (0, 2] are
 * dm_lsm_refine's.  radius r in [2, 7] (at r = 1 nine taps cannot carry eight unknowns), n =
 * (2r+1)^2.  max_shear in (0, 1).  Float64 throughout, one rounding per operation, no contraction;
 * an expression is evaluated as its parentheses say and otherwise left to right.  Sums over the
 * window run v outer, u inner, both ascending ("raster order").  Per cell (y, x), (cy, cx) =
 * (y + oy, x + ox):
 *   1. Skip and halo rule: dm_lsm_refine's rule 1.  A skipped cell copies both planes bit for bit;
 *      its status is 0, its score and its four affine values are NaN (0x7ff8000000000000).
 *   2. Once per cell, as exact integers: A(u, v) = img1[cy+v][cx+u], Gx = A(u+1, v) - A(u-1, v),
 *      Gy = A(u, v+1) - A(u, v-1) (doubled central differences, read from the halo), the six
 *      regressors phi = (Gx, Gx u, Gx v, Gy, Gy u, Gy v), and
 *        sa = sum A, VA = n sum A^2 - sa^2, f_k = sum phi_k,
 *        N_kl = n sum(phi_k phi_l) - f_k f_l (k >= l: 21 values), RA_k = n sum(phi_k A) - f_k sa.
 *      |phi| <= 255 * 7, so every one is below 2^53 in magnitude and converts to double exactly.
 *   3. N = L D L^T in double, column by column: for j = 0 .. 5, for i = j .. 5:
 *        c_ij = N_ij, then for k = 0 .. j-1 in turn c_ij = c_ij - L_ik * c_jk;
 *        d_j = c_jj; the pivot passes if d_j > N_jj * 2^-20 (a NaN fails); L_ij = c_ij / d_j (i > j).
 *      The first pivot that fails ends the cell: status -1, score and affine NaN, the input is kept.
 *      2^-20 is a condition, not a measurement: a pivot is what is left of a regressor's variance
 *      once the earlier regressors are taken out, and double carries 53 bits.
 *   4. (py0, px0) = ((double)cy - d_row, (double)cx - d_col).  If it fails dm_photo_score's rule 3
 *      (r <= py0 < Hi-r-1 and r <= px0 < Wi-r-1, on the double): status -2, score and affine NaN,
 *      the input is kept.  Else s0 is dm_photo_score's score at (py0, px0), bit for bit.
 *   5. The parameters are (px, a, b, py, c, d), the order of phi; they start at (px0, 0, 0, py0, 0, 0).
 *      "The warp passes" if the four taps (u, v) = (-r,-r), (r,-r), (-r,r), (r,r) satisfy 0 <= Y <
 *      Hi - 1 and 0 <= X < Wi - 1, with 1 + a and 1 + d formed once as 1.0 + a and 1.0 + d and X, Y
 *      as written above (u and v converted to double).  Rounding is monotone, so every tap of a
 *      warp that passes lies inside as well.  If the starting warp does not pass: status -2, the
 *      score s0, the input is kept.  The sums of a warp, over the taps in raster order: the sample
 *      is P = ((w0 B00 + w1 B01) + w2 B10) + w3 B11 with dm_photo_score's corner iy = floor(Y), ix =
 *      floor(X) and weights (rule 5 there: fy = Y - iy, fx = X - ix, w0 = (1-fy) * (1-fx), w1 =
 *      (1-fy) * fx, w2 = fy * (1-fx), w3 = fy * fx) and B00 = img2[iy][ix], B01 = img2[iy][ix+1],
 *      B10 = img2[iy+1][ix], B11 = img2[iy+1][ix+1]; then
 *        Sp = Sp + P, Spp = Spp + P * P, Sap = Sap + A * P, T_k = T_k + phi_k * P (k = 0 .. 5)
 *      (A and phi_k converted to double; all sums start at 0.0), and
 *        num = n * Sap - sa * Sp,   vb = n * Spp - Sp * Sp.
 *      Step t = 1 .. iters: the sums of the current warp.  Unless vb > 0: status -1, the score s0,
 *      the input is kept.  Else
 *        alpha = num / vb,   rhs_k = RA_k - alpha * (n * T_k - f_k * Sp),
 *        z_i = rhs_i, then for k = 0 .. i-1 in turn z_i = z_i - L_ik * z_k          (i = 0 .. 5)
 *        q_i = z_i / d_i, then for k = i+1 .. 5 in turn q_i = q_i - L_ki * delta_k   (i = 5 .. 0;
 *        delta_i is the final q_i)
 *      and every parameter moves by 2.0 * delta_k: px = px + 2.0 * delta_0, a = a + 2.0 * delta_1,
 *      b, py, c, d likewise.  Unless |px - px0| <= max_move, |py - py0| <= max_move, |a|, |b|, |c|,
 *      |d| <= max_shear and the new warp passes (a NaN fails every test): status -2, the score s0,
 *      the input is kept.
 *   6. With the sums of the final warp (T_k not needed), s1 = the score of dm_photo_score's rule 5
 *      from VA, num and vb: 0.0 unless VA > 0 and vb > 0, else num / sqrt(VA * vb) clamped to
 *      [-1, 1].  s1 > s0: the cell is accepted, status = iters, out_row = (double)cy - py, out_col =
 *      (double)cx - px, the score s1, the affine values (a, b, c, d).  Else status -3, the input bits
 *      are kept, the score s0, the affine values NaN.  A cell that ended with -1 or -2 in rule 5
 *      has the score s0 and the affine values NaN.
 *   7. A cell reads only its own d_row and d_col, before it writes: d_out_row and d_out_col may
 *      alias d_row and d_col.  The result depends on nothing but the cell.
 * The factor 2.0 undoes the doubling of the differences, as in dm_lsm_refine.  It follows that a
 * cell on identical windows at an integer disparity has P = A exactly, alpha = 1.0, rhs = 0 and
 * status -3 (it never moves), that an accepted cell scores strictly above dm_photo_score of the
 * input, and that an unaccepted scored cell reports dm_photo_score's bits.
 * tests/test_lsm_affine_host.py restates this in plain loops; the kernel equals it bit for bit. */
#ifndef DMSTEREO_LSM_H
#define DMSTEREO_LSM_H

#include "dmstereo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace dm_lsm_affine asks for (a constant 16: the kernel keeps everything on
 * chip); 0 for a shape it does not take: dm_photo_bytes' limits on H, W, Hi or Wi above 2^30, a
 * radius outside [2, 7] or iters outside [1, 8]. */
size_t dm_lsm_affine_bytes(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t iters);

/* d_mask (uint8 [H][W]), d_score (float64 [H][W]), d_status (int8 [H][W]) and d_affine (float64
 * [4][H][W]: a, b, c, d) may be NULL.  d_work: dm_lsm_affine_bytes(...) bytes, not NULL.  flags
 * must be 0.  DM_ERR_ARG for a null image / plane / output / workspace, a side below 1, a stride
 * below Wi, an offset outside [-2^30, 2^30], a radius outside [2, 7], iters outside [1, 8], a
 * max_move outside (0, 2] or a max_shear outside (0, 1) (NaN included), a flag bit;
 * DM_ERR_UNSUPPORTED for the other shapes dm_lsm_affine_bytes refuses.  Validation precedes every
 * HIP call; nothing is allocated, nothing synchronises, one launch on `stream`; the result is the
 * same from run to run. */
int dm_lsm_affine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2,
                  int32_t Hi, int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W,
                  int32_t oy, int32_t ox, int32_t radius, int32_t iters, double max_move, double max_shear,
                  int32_t flags, const uint8_t *d_mask /* may be NULL */, double *d_out_row,
                  double *d_out_col, double *d_score /* may be NULL */, int8_t *d_status /* may be NULL */,
                  double *d_affine /* may be NULL */, void *d_work, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DMSTEREO_LSM_H */
