/* dmstereo_sgm.h -- semi-global re-matching of a disparity map (csrc/dm_sgm.hip).
 *
 * A second public header of libdmstereo.so, beside dmstereo.h, whose status codes it uses;
 * dm_abi_version() does not change with it.
 *
 * Not in the reference.  dm_photo_refine measures every cell on its own: where the images say
 * little (low texture under noise, repeated structure) its argmax takes whichever candidate the
 * noise favours.  dm_sgm_refine decides the cells of a map together: the matching costs of the
 * (2s+1)^2 integer candidates of every cell and a smoothness term between neighbouring cells are
 * minimised along 4 or 8 scan directions and summed (Hirschmueller's semi-global matching), over
 * this project's two-axis disparities.
 *
 * Inputs.  Images, planes d_row / d_col, offsets oy, ox and the radius r in [1, 7] are
 * dm_photo_score's (dmstereo.h).  `search` is s in [1, 3]: NC = 2s+1, L = NC^2 labels a = (ay, ax)
 * in [-s, s]^2, label index (ay+s) NC + (ax+s).  `paths` is 4 or 8.  p1, p2: integer penalties,
 * 0 <= p1 <= p2 <= 16384, in cost units of 1/1024 of a score.  flags: DM_SGM_SUBPIX.  d_mask:
 * optional, uint8 [H][W].  Per cell (y, x), (cy, cx) = (y + oy, x + ox):
 *   1. Cell states.  py = (double)cy - d_row, px = (double)cx - d_col.  The cell is DEAD if a
 *      disparity is not finite (the range test on the double) or py or px lies outside
 *      [-2^30, 2^30] (tested on the double, before any conversion).  Otherwise by =
 *      (int64)rint(py), bx = (int64)rint(px), ties to even, and the cell's base displacement is
 *      (by - cy, bx - cx) in int64.  The cell is FIXED if it is not dead, d_mask is given and it
 *      is 0 at the cell; every other cell is FREE.
 *   2. Costs, uint16.  Candidate a of a free cell is scored iff the img1 window, rows cy-r .. cy+r
 *      and columns cx-r .. cx+r, lies in the image, r <= by+ay <= Hi-r-2 and r <= bx+ax <=
 *      Wi-r-2.  With A the img1 window, P the img2 window centred on (by+ay, bx+ax), n = (2r+1)^2
 *      and dm_photo_score's exact integer sums:
 *        CA = n sum(A P) - sum A sum P,  VA = n sum A^2 - (sum A)^2,  CB = n sum P^2 - (sum P)^2,
 *      the score is 0.0 unless VA > 0 and CB > 0; else t = CA / sqrt(VA * CB) clamped to [-1, 1]
 *      (float64, one rounding per operation, no contraction).  This is dm_photo_score's score at
 *      the integer disparity (cy - by - ay, cx - bx - ax), bit for bit: its weights are 1, 0, 0, 0
 *      there.  C(p, a) = (int)rint((1.0 - score) * 1024.0), in [0, 2048].  An unscored candidate
 *      of a free cell costs 2048.  A fixed cell costs 0 at label (0, 0) and 32768 at every other
 *      label; nothing is read from the images for it.
 *   3. Paths.  The directions rho are, in this order, (0,1), (0,-1), (1,0), (-1,0) and with
 *      paths = 8 also (1,1), (1,-1), (-1,1), (-1,-1) (row step, column step).  The predecessor of
 *      p is q = p - rho.  If q is outside the map or dead, L_rho(p, a) = C(p, a); else
 *        L_rho(p, a) = C(p, a) + min_b [L_rho(q, b) + V] - min_b L_rho(q, b),
 *      where V is 0, p1 or p2 as the Chebyshev distance between the displacements
 *      (by_p + ay - cy_p, bx_p + ax - cx_p) of label a at p and (by_q + by' - cy_q, bx_q + bx' -
 *      cx_q) of label b = (by', bx') at q is 0, 1 or more.  A dead cell has no L.  Everything is
 *      an integer; L_rho <= 32768 + p2; S(p, a) = sum_rho L_rho(p, a) fits uint32.  Integer sums
 *      do not depend on the order of accumulation: that is why the costs are quantised.
 *   4. Winner.  The winner of a free cell is the scored candidate with the smallest S; ties go to
 *      the smallest ay^2 + ax^2, then the smaller ay, then the smaller ax.
 *   5. Output.  A dead cell, a fixed cell, a free cell without a scored candidate and a free cell
 *      whose winner is (0, 0) copy both planes bit for bit (NaN payloads and -0.0 included); their
 *      shift is (0, 0).  Another winner (ay, ax) gives out_row = (double)(cy - by - ay) - ty,
 *      out_col = (double)(cx - bx - ax) - tx and the shift (ay, ax).  ty = tx = 0.0 unless
 *      DM_SGM_SUBPIX is set; with it, per axis, if both neighbours of the winner along the axis
 *      lie in [-s, s] and are scored, with sums Sm (at -1) and Sp (at +1) and the winner's S0:
 *      den = (Sm + Sp) - 2 S0 (int64), and if den > 0, t = (0.5 * (double)(Sm - Sp)) / (double)den,
 *      clamped to [-0.5, 0.5].  The score output is the winner's score (candidate (0, 0)'s if that
 *      wins); NaN (0x7ff8000000000000) for dead cells, fixed cells and cells with no scored
 *      candidate.
 *   6. Aliasing and determinism.  d_out_row / d_out_col may alias d_row / d_col: every input
 *      plane and the mask are read into the workspace (bases and states) before any output is
 *      written, and a cell copies its own bits only.  The result is the same from run to run.
 * tests/test_sgm_host.py restates this in plain loops; the kernels equal it bit for bit. */
#ifndef DMSTEREO_SGM_H
#define DMSTEREO_SGM_H

#include "dmstereo.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { DM_SGM_SUBPIX = 1 };

/* Bytes of the workspace dm_sgm_refine asks for: the costs (uint16), the sums S (uint32), the
 * base displacements (int64) and the states of H x W cells with (2 search + 1)^2 labels; 0 for a
 * shape it does not take: dm_photo_bytes' limits on H, W, a search outside [1, 3], paths other
 * than 4 or 8, or a workspace that does not fit size_t. */
size_t dm_sgm_bytes(int32_t H, int32_t W, int32_t search, int32_t paths);

/* d_mask (uint8 [H][W]), d_score (float64 [H][W]) and d_shift (int8 [2][H][W]: ay, then ax) may be
 * NULL.  d_work: dm_sgm_bytes(H, W, search, paths) bytes, 16-byte aligned, not NULL.  DM_ERR_ARG
 * for a null image / plane / output / workspace, a side below 1, a stride below Wi, an offset
 * outside [-2^30, 2^30], a radius outside [1, 7], a search outside [1, 3], paths other than 4 or
 * 8, penalties outside 0 <= p1 <= p2 <= 16384, unknown flag bits; DM_ERR_UNSUPPORTED for the other
 * shapes dm_sgm_bytes refuses and for images above 2^30 a side.  Validation precedes every HIP
 * call; nothing is allocated, nothing synchronises; three launches and one hipMemsetAsync on
 * `stream`. */
int dm_sgm_refine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2,
                  int32_t Hi, int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W,
                  int32_t oy, int32_t ox, int32_t radius, int32_t search, int32_t paths, int32_t p1,
                  int32_t p2, int32_t flags, const uint8_t *d_mask /* may be NULL */, double *d_out_row,
                  double *d_out_col, double *d_score /* may be NULL */, int8_t *d_shift /* may be NULL */,
                  void *d_work, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DMSTEREO_SGM_H */
