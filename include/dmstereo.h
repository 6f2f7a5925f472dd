/*
 * dmstereo.h -- C ABI of the MI355X (gfx950) DeepMatching stereo correlation engine.
 *
 * The reference path this ABI replaces is Python (Yuki-Kumon/deepmatching_stereo_matching):
 *   misc/Correlation_map.py  Correlation_map (:29-173), Maxpool (:176-184)
 *   misc/Feature_value.py    Feature_value (:18-43) -> cv2.matchTemplate + min_max
 *   misc/Matching.py         Matching (:20-255), Zero_padding (:258-268)
 *   misc/Calc_difference.py  Calc_difference.cal_map (:26-49)
 *   misc/sub_pix_cal.py      sub_pix_cal (:22-53)
 *   misc/image_cut_solver.py ImageCutSolver._execute_matching stitching (:144-179)
 *   misc/optimize_loop.py    optimize_loop (:15-37), image_threshold (:40-44)
 *   misc/opt_loop.py         optimize_loop_bilateral_* (:16-58), make_weight (:60-85)
 * The Python mirror of that surface (deepmatching_stereo_matching_amd/misc/) binds
 * these entry points with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Every pointer argument named d_* is DEVICE memory owned by the caller (torch
 *    tensors in the Python host).  The library never allocates or frees device memory
 *    and keeps no global mutable state besides a per-thread error string.
 *  - Work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *    and is asynchronous; nothing here synchronises.
 *  - Return 0 (DM_OK) or a negative dm_status; dm_last_error() describes the failure.
 *
 * Shapes.  A batch holds T tiles of equal size cut from one image pair.  For tile t the
 * crop is rows [org_t.r, org_t.r + h0 + ws - 1) x cols [org_t.c, org_t.c + w0 + ws - 1) of
 * img1 and img2 (the same window in both, as ImageCutSolver._cut_and_pool does,
 * image_cut_solver.py:95-113).  h0 = H' and w0 = W' are the correlation-map sides
 * (Correlation_map: H' = H - 2*exclusive_pix).  P = h0*w0.
 *  level 0  : "co_map", float32 [T][P][P] (min-max normalised, NOT rectified)
 *  level l>0: float64 [T][Pl][Pl], Pl = (h0>>l)*(w0>>l), rectified (**1.4) like
 *             co_map_list[l].
 */
#ifndef DMSTEREO_H
#define DMSTEREO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum dm_status {
    DM_OK = 0,
    DM_ERR_ARG = -1,         /* bad pointer / size argument                              */
    DM_ERR_SHAPE = -2,       /* shape the reference cannot process (even ws, odd sides) */
    DM_ERR_UNSUPPORTED = -3, /* valid for the reference, not (yet) for this engine      */
    DM_ERR_HIP = -4          /* a HIP runtime call failed                               */
};

enum dm_method { /* cv2 constants, Feature_value.py:23-30 */
    DM_TM_CCOEFF = 4,
    DM_TM_CCOEFF_NORMED = 5
};

enum dm_cal_mode { /* Calc_difference.cal_map modes, Calc_difference.py:30 */
    DM_CAL_ELEVATION = 0,  /* j - map[1] */
    DM_CAL_ELEVATION2 = 1, /* i - map[0] */
    DM_CAL_DISTANCE = 2    /* || (i, j) - map[:2] || */
};

typedef struct dm_tiles {
    const uint8_t *d_img1;    /* "img" / original / before   (Correlation_map arg 1) */
    const uint8_t *d_img2;    /* "template" / after          (Correlation_map arg 2) */
    int32_t pitch1, pitch2;   /* row pitch in bytes                                   */
    const int32_t *d_origins; /* [T][2] crop top-left (row, col)                      */
    int32_t T;                /* tiles in the batch                                    */
    int32_t h0, w0;           /* correlation-map sides                                 */
    int32_t ws;               /* window_size, odd, 1..15                               */
    int32_t method;           /* dm_method                                             */
} dm_tiles;

/* Size in bytes of the per-batch statistics workspace: per-patch / per-window moments and
 * the per-patch min/max of the level-0 map (6 * 4 * T * P), plus, for shapes the MFMA
 * kernels take, the window operands in MFMA fragment order (T * h0 * (w0/16) * (KS*1024
 * + 128), KS = ceil(ws^2 / 64)), and for ws <= 5 a second such region in the volume
 * kernels' column-group layout (dm_corr_volume and dm_corr_volume_f16 fill it themselves). */
size_t dm_stats_bytes(const dm_tiles *b);

/* Per-patch and per-window moments.
 * Replaces Correlation_map._create_atomic_patch (Correlation_map.py:51-67) and the
 * template/window sums inside cv2.matchTemplate (Feature_value.py:41). */
int dm_corr_stats(const dm_tiles *b, void *d_stats, void *stream);

/* Level-0 ZNCC + per-patch min-max + rectification + MaxPool(3,2,1) + 4-child average +
 * rectification, fused: writes level 1 (float64 [T][P1][P1]) and the per-patch min/max
 * into d_stats.  Level 0 is never written.
 * Replaces Correlation_map._create_simple_initial_co_map (:69-87), Feature_value.min_max
 * (Feature_value.py:32-37), _rectification (:158-159) and the first _aggregation
 * (:89-130) of _multi_level_correlation_pyramid (:132-156).  Needs dm_corr_stats first. */
int dm_corr_level1(const dm_tiles *b, void *d_stats, double *d_level1, void *stream);

/* dm_corr_level1 followed by the second _aggregation (Correlation_map.py:89-130, :148-153)
 * in the same kernel: writes level 2 (float64 [T][P2][P2], P2 = (h0/4)*(w0/4)) and, when
 * d_level1 is non-NULL, level 1 as well.  With d_level1 NULL level 1 never reaches HBM;
 * dm_match then evaluates it on demand.  Needs h0 % 4 == 0, w0 in {32,64,128,256},
 * ws <= 15 (DM_ERR_UNSUPPORTED otherwise: use dm_corr_level1 + dm_aggregate). */
int dm_corr_level12(const dm_tiles *b, void *d_stats, double *d_level1, double *d_level2, void *stream);

/* Materialise the level-0 min-max volume "co_map" (float32 [T][P][P]) and the per-patch
 * min/max.  Replaces _create_simple_initial_co_map (:69-87) for callers that read
 * co_map directly (bad_matching.py:62-70).  Needs dm_corr_stats first.  d_l0 must be 16-byte
 * aligned, here and in dm_corr_volume_f16 and dm_corr_volume_ex (the MFMA kernels store 16 bytes
 * per lane): DM_ERR_ARG otherwise, before any HIP call. */
int dm_corr_volume(const dm_tiles *b, void *d_stats, float *d_l0, void *stream);

/* dm_corr_volume with a binary16 volume (uint16_t bit patterns, [T][P][P]): each float32
 * co_map value rounded to nearest-even half, i.e. np.float16(co_map).  The fp16
 * correlation volume of BASELINE config C5 (2 B/voxel instead of 4); not bit-exact with
 * the reference by construction (SURVEY.md 8(a) parity rules: a flip rate is reported).
 * Needs dm_corr_stats first. */
int dm_corr_volume_f16(const dm_tiles *b, void *d_stats, uint16_t *d_l0, void *stream);

/* Flags of dm_corr_volume_ex. */
enum {
    DM_VOLUME_F16 = 1,            /* binary16 output (dm_corr_volume_f16), else float32     */
    DM_VOLUME_MINMAX_KNOWN = 2    /* d_stats already holds the per-patch min/max: written by
                                     dm_corr_level1 / dm_corr_level12 / a volume call on the
                                     same tiles and stats.  The kernel then skips its own
                                     min/max sweep (the same values: bit-identical output).  */
};

/* dm_corr_volume / dm_corr_volume_f16 with flags: the same level-0 volume, and, with
 * DM_VOLUME_MINMAX_KNOWN, without re-deriving the per-patch min/max that an earlier call
 * left in d_stats -- the reference's co_map read after Correlation_map()() has built the
 * pyramid (bad_matching.py:62-70 reads it before; Correlation_map.py:69-87 computes both
 * in one pass).  d_l0: float * or uint16_t * by DM_VOLUME_F16. */
int dm_corr_volume_ex(const dm_tiles *b, void *d_stats, int32_t flags, void *d_l0, void *stream);

/* d_out[i] = (double)half(d_in[i]) ** 1.4: _rectification (:158-159) of an fp16 volume. */
int dm_rectify_f16(const uint16_t *d_in, size_t n, double *d_out, void *stream);

/* d_out[i] = d_in[i] ** 1.4 (pinned float64 pow, dm_pow.h).  Replaces
 * Correlation_map._rectification (:158-159) for the materialised co_map_list[0]. */
int dm_rectify(const float *d_in, size_t n, double *d_out, void *stream);

/* Same for float64 input (Correlation_map._rectification on an aggregated map). */
int dm_rectify64(const double *d_in, size_t n, double *d_out, void *stream);

/* Self-test of the pow14 forms the fused kernels evaluate in place of _rectification
 * (:158-159), tables in LDS as the kernels hold them.  d_out[i] = form(d_in[i]); each form
 * equals dm_pow14 (dm_pow.h) bit for bit on its domain, and only there:
 *   DM_POW_F32   pow14_zf((float)x): 0, NaN and float32-normal x in (0, 1] (the level
 *                kernel's child values: x is a float32 in [0, 1] or NaN)
 *   DM_POW_Q4    pow14_q4(s) = pow14(s / 4): s == 0, NaN, or s / 4 in [2^-319, 1] (a sum of
 *                four children, level-1 / level-2 averaging); 0 < s / 4 < 2^-319 gives 0 and
 *                s = +inf NaN instead of dm_pow14's values
 *   DM_POW_K     pow14_k(x): 0, NaN and x in [2^-319, 1]
 *   DM_POW_FULL  pow14_lds(x): every double (the slow path outside [2^-319, 1])
 * Any other variant (4 and 5, the pruned level kernel's forms of ABI 1.10, included: that kernel
 * was removed) fails with DM_ERR_ARG. */
enum dm_pow_variant { DM_POW_F32 = 0, DM_POW_Q4 = 1, DM_POW_K = 2, DM_POW_FULL = 3 };
int dm_pow14_variant(int32_t variant, const double *d_in, size_t n, double *d_out, void *stream);

/* Self-test of the exact float32 num = n * sum_k T'_k I'_k - sum(T') * sum(I') from ONE
 * v_mfma_f32_16x16x32_f16 (csrc/dm_mfma.h, num_tile_f16), through the device helpers a level
 * kernel would use: the binary16 operand builders, the digit split of the sums and the MFMA
 * call.  d_patch_taps / d_window_taps: uint8 [16][ws*ws] (tap k = ws * row + column; T' and
 * I' are the bytes - 128); d_num: float32 [16 patches][16 windows].  ws in {1, 3, 5}
 * (ws*ws + 4 of the instruction's 32 K slots).  Every d_num equals the integer exactly. */
int dm_debug_num_tile_f16(const uint8_t *d_patch_taps, const uint8_t *d_window_taps, int32_t ws,
                          float *d_num, void *stream);

/* 1 when the level kernel of this batch (dm_corr_level1 / dm_corr_level12) takes num from the
 * f16 MFMA in its second sweep, 0 otherwise: the one predicate by which dm_corr_stats chooses
 * the window-operand layout and the launcher the kernel instance (w0 = 128, ws <= 5,
 * h0 % 4 == 0 in a default build).  Reads the shape fields of *b only, no device memory. */
int dm_level_num_f16(const dm_tiles *b);

/* One pyramid step for levels >= 1: MaxPool2d(3,2,1) per map, (ul+ur+ll+lr)/4, and
 * (rectify != 0) the 1.4 power.  d_in float64 [T][h*w][h*w] -> d_out float64
 * [T][(h/2)*(w/2)][(h/2)*(w/2)].
 * Replaces Correlation_map._aggregation (:89-130) [+ _rectification (:148)]. */
int dm_aggregate(const double *d_in, int32_t T, int32_t h, int32_t w, int32_t rectify,
                 double *d_out, void *stream);

/* Coarse-to-fine matching on a pyramid of nlev levels of T tiles with level-0 sides
 * h0 x w0.  d_levels is a HOST array of nlev device pointers to float64 rectified levels
 * (co_map_list).  d_levels[0] may be NULL: level 0 is then evaluated on demand from the
 * images and the statistics (b and d_stats required; b->T/h0/w0 must match).  When
 * d_levels[0] is NULL and nlev >= 3, d_levels[1] may be NULL as well (level 1 on demand,
 * for a pyramid built by dm_corr_level12 without level 1).
 * filter_num > 0 runs Matching._filter (:224-255; filter_mode 0 average, 1 median, window
 * filter_window <= 7, square maps only) after the top level and after each _B step while
 * the count lasts, as Matching._initial_move_map / _B do.
 * d_scratch: float64 [T][3][h0*w0].  d_out: float64 [T][3][h0][w0] = (row, col, score),
 * as returned by Matching.__call__ (Matching.py:211-222): _initial_move_map (:80-96),
 * _B/_calc_match (:98-149), _calc_near_match (:58-78), _sub_pix_cal (:177-209). */
int dm_match(const dm_tiles *b, const void *d_stats, const double *const *d_levels,
             int32_t nlev, int32_t T, int32_t h0, int32_t w0, int32_t sub_pix,
             int32_t filter_window, int32_t filter_num, int32_t filter_mode,
             double *d_scratch, double *d_out, void *stream);

/* Matching._sub_pix_cal (Matching.py:177-209) for a descent that stops ABOVE level 0 (an
 * N_map whose halvings end before the list does, Matching.py:85-96, :133-134): the final
 * map of a coarser level (float64 [T][3][hm][wm], from dm_match on co_map_list[bottom:]
 * without sub_pix) is refined in place against the materialised level 0 d_level0 (float64
 * [T][h0*w0][h0*w0], co_map_list[0]) at patch (i, j) and window (row, col) of each entry, as
 * the reference does; bounds are level 0's (h0, w0).  Any map is accepted and indexed as numpy
 * indexes co_map_list[0] (Matching.py:186-188, :199-201): c = int(entry), an index in [-N, N)
 * is valid and a negative one wraps, any other raises IndexError and takes the bare except
 * (:193-194, :205-206: i - d_x, j - d_y).  hm <= h0, wm <= w0.  dm_match's own sub_pix is
 * this with hm = h0, wm = w0. */
int dm_subpix_map(const double *d_level0, int32_t T, int32_t h0, int32_t w0, int32_t hm, int32_t wm,
                  double *d_map, void *stream);

/* The same refinement with level 0 evaluated on demand (ABI 1.9): the five level-0 values an
 * entry reads are recomputed from the tile batch's images and the statistics workspace of
 * dm_corr_stats + dm_corr_level1/12 (its per-patch min / max), exactly as dm_match's own
 * sub-pixel step does, so a descent that stops above level 0 never materialises
 * co_map_list[0] (T * (h0 w0)^2 float64).  d_map: float64 [b->T][3][hm][wm], in place. */
int dm_subpix_map_tiles(const dm_tiles *b, const void *d_stats, int32_t hm, int32_t wm, double *d_map,
                        void *stream);

/* misc/sub_pix_cal.py sub_pix_cal (:22-53): clamp to [-3,3], quadratic refinement of an
 * (h, w) disparity map along `direction` (0 rows, 1 cols) on the score map scaled by
 * `ratio`, reject |delta| > 1, clamp again.  float64 in/out, device pointers. */
int dm_sub_pix_cal(const double *d_arr, const double *d_score, int32_t h, int32_t w,
                   int32_t direction, double ratio, double *d_out, void *stream);

/* Calc_difference.cal_map (Calc_difference.py:26-49) on T maps [T][3][h][w] -> [T][h][w]. */
int dm_cal_map(const double *d_map, int32_t T, int32_t h, int32_t w, int32_t mode,
               double *d_out, void *stream);

/* ImageCutSolver stitching (image_cut_solver.py:144-179): tiles t = j*n0 + i of d_match
 * ([T][3][h0][w0]) are written at (stride0*i, stride1*j), later tiles overwriting
 * earlier ones.  d_dmap: [nmodes][Hout][Wout] (cal_map of each mode in `modes`, a HOST
 * array), d_score: [Hout][Wout] (map[2]).  Hout = stride0*(n0-1)+h0, likewise Wout.
 * Output cells no tile covers are NaN (np.empty garbage in the reference). */
int dm_stitch(const double *d_match, int32_t n0, int32_t n1, int32_t h0, int32_t w0,
              int32_t stride0, int32_t stride1, const int32_t *modes, int32_t nmodes,
              double *d_dmap, double *d_score, void *stream);

/* ---- Forward-backward consistency check (dm_fb.hip) -------------------------------------
 * Not in the reference, whose only confidence signal is map[2] (level 0 is min-max
 * normalised per patch, so every patch's best match scores 1.0).  d_fwd holds the tiles of
 * img1 matched into img2, d_bwd img2 matched into img1: both float64 [T][3][h][w] as dm_match
 * writes them, tile-local coordinates, the same crop window in both images
 * (ImageCutSolver._cut_and_pool, image_cut_solver.py:95-113).  For tile t, cell (i, j), in
 * float64 without contraction:
 *   qi = floor(F[t,0,i,j] + 0.5);  qj = floor(F[t,1,i,j] + 0.5)
 *   err = NaN                                         unless 0 <= qi < h and 0 <= qj < w
 *   err = || B[t,0:2,qi,qj] - (i, j) ||               otherwise
 *   valid = err <= tol                                (false for NaN)
 * The range test is made on the doubles before any conversion to int: NaN, +-inf and
 * off-tile matches give err = NaN and are never used as an index. */

/* The check on T tiles: d_err [T][h][w] receives err; d_masked ([T][3][h][w], may be NULL)
 * the forward map with rows 0 and 1 set to NaN at invalid cells and row 2 (the score)
 * copied.  d_masked may equal d_fwd (masking in place: a thread reads only its own forward
 * cell); d_err must not overlap the inputs.  tol >= 0, +inf allowed (DM_ERR_ARG for a
 * negative or NaN tolerance). */
int dm_fb_check(const double *d_fwd, const double *d_bwd, int32_t T, int32_t h, int32_t w,
                double tol, double *d_err, double *d_masked, void *stream);

/* dm_stitch of the forward tiles with the check fused in: each output pixel picks its tile
 * by dm_stitch's rule (later tiles overwrite earlier ones), evaluates the check at its tile
 * cell, and writes every d_dmap mode as NaN where the cell is invalid and as dm_stitch's
 * value otherwise, d_score = map[2] unchanged, and d_err [Hout][Wout] = err.  Output cells
 * no tile covers are NaN in all three.  Equals dm_fb_check (masked) followed by dm_stitch. */
int dm_stitch_fb(const double *d_fwd, const double *d_bwd, int32_t n0, int32_t n1, int32_t h0,
                 int32_t w0, int32_t stride0, int32_t stride1, const int32_t *modes,
                 int32_t nmodes, double tol, double *d_dmap, double *d_score, double *d_err,
                 void *stream);

/* ---- Overlap-merging stitch (dm_merge.hip) -------------------------------------------------
 * Not in the reference.  dm_stitch and dm_stitch_fb keep the LAST tile that covers an output
 * pixel; with overlapping tiles (stride S / 2: four solves per interior pixel) the other
 * estimates are discarded.  dm_stitch_merge takes every covering tile as a candidate.  d_fwd
 * and d_bwd (may be NULL: a one-direction solve) are dm_stitch_fb's.  All arithmetic is float64
 * without contraction, in the order written.
 *
 * Candidates.  Output pixel (y, x) has as candidates every tile (i, j) with
 * 0 <= y - i*stride0 < h0 and 0 <= x - j*stride1 < w0, enumerated with j as the outer loop and
 * i as the inner loop, both ascending: the tile index t = j*n0 + i ascends, the order dm_stitch
 * overwrites in.  For candidate c the local cell is (ly, lx) = (y - i*stride0, x - j*stride1);
 *   r = F[t,0,ly,lx], q = F[t,1,ly,lx], s = F[t,2,ly,lx]
 *   e_c     = err of the forward-backward check above at tile t, cell (ly, lx) when d_bwd is
 *             given (indices are formed only from doubles that passed the range test)
 *   valid_c = isfinite(r) && isfinite(q) && (d_bwd == NULL || e_c <= tol)
 *   v_c,k   = dm_stitch's value of mode k: lx - q, ly - r, or sqrt(a*a + b*b) of a = ly - r,
 *             b = lx - q
 *   g_c     = min(ly + 1, h0 - ly) * min(lx + 1, w0 - lx)   (the distance to the tile's edge,
 *             rows times columns: an exact integer, formed as a product of two doubles)
 * m is the number of valid candidates.
 *
 * Rules.
 *   DM_MERGE_LAST     bit for bit dm_stitch when d_bwd is NULL (the last candidate's values
 *                     whatever they are) and dm_stitch_fb when it is given.  min_count must be 1.
 *   DM_MERGE_CENTER   the valid candidate with the largest g, ties to the later candidate:
 *                     value, score and err are that candidate's.
 *   DM_MERGE_FEATHER  num = 0, den = 0; for each valid c in order num = num + g_c*v_c,
 *                     den = den + g_c; the output is num / den.  The score likewise over s_c.
 *   DM_MERGE_MEDIAN   rank(c) = #{c' valid : v' < v or (v' == v and c' < c)}.  Odd m: the value
 *                     at rank (m-1)/2; even m: (a + b) * 0.5 of the values at ranks m/2 - 1 and
 *                     m/2.  Per mode, and the score likewise over s_c.  (The value "at" a rank
 *                     is that of the last candidate in order with that rank, NaN if none has it:
 *                     the ranks are a permutation unless some s_c is NaN.)
 * Rules 1 to 3: when m < min_count every dmap mode is NaN.  When m == 0 on a covered pixel the
 * score and err are the last covering candidate's, as dm_stitch_fb leaves them; otherwise err
 * is the minimum e_c over the valid candidates, except for CENTER (the chosen candidate's).
 *
 * Outputs, every rule: d_count [H][W] = m; d_spread [nmodes][H][W] = max - min of v_c,k over
 * the valid candidates, NaN for m == 0.  A pixel no tile covers is NaN in every float output
 * and 0 in d_count.  d_err, d_spread and d_count may be NULL.
 *
 * Validation precedes any HIP call and is dm_stitch_fb's, and: rule in 0..3; 1 <= min_count
 * <= 255; a non-NULL d_err with a NULL d_bwd is DM_ERR_ARG; tol is checked only when d_bwd is
 * given; min(n0, ceil(h0/stride0)) * min(n1, ceil(w0/stride1)) > DM_MERGE_MAX_CAND (more tiles
 * over one pixel than the kernel's candidate mask holds) is DM_ERR_UNSUPPORTED. */
enum dm_merge_rule { DM_MERGE_LAST = 0, DM_MERGE_CENTER = 1, DM_MERGE_FEATHER = 2, DM_MERGE_MEDIAN = 3 };
#define DM_MERGE_MAX_CAND 64
int dm_stitch_merge(const double *d_fwd, const double *d_bwd /* may be NULL */,
                    int32_t n0, int32_t n1, int32_t h0, int32_t w0, int32_t stride0, int32_t stride1,
                    const int32_t *modes, int32_t nmodes, double tol, int32_t rule, int32_t min_count,
                    double *d_dmap, double *d_score, double *d_err /* may be NULL */,
                    double *d_spread /* [nmodes][H][W], may be NULL */, uint8_t *d_count /* [H][W], may be NULL */,
                    void *stream);

/* ---- Hole fill (dm_fill.hip) -------------------------------------------------------------
 * Not in the reference.  dm_stitch leaves NaN where no tile covers and dm_stitch_fb where the
 * round trip misses, and one NaN poisons every cell the Gauss-Seidel sweeps below visit after
 * it.  dm_fill_holes makes a map dense: cascadic push-pull with masked Jacobi relaxation,
 * deterministic, each of the M maps of d_in [M][H][W] from its own holes.  A hole is a
 * non-finite cell (NaN, +-inf; the range test is made on the double).  Level 0 is the map
 * with (v, n) = (x, 1) at finite cells and (0, 0) at holes; level k + 1 has sides
 * ceil(h / 2), ceil(w / 2).  In float64 without contraction, in the order written:
 *   pull   s = ((n00 v00 + n01 v01) + n10 v10) + n11 v11;  m = ((n00 + n01) + n10) + n11
 *          v' = m > 0 ? s / m : 0;  n' = m         (children outside the level: v = n = 0)
 *   push   a cell with n == 0 takes (((9 a + 3 b) + 3 c) + d) * 0.0625 of the finished level
 *          k + 1: a = p[I][J], b = p[I2][J], c = p[I][J2], d = p[I2][J2], I = i >> 1,
 *          I2 = I + 1 for odd i and I - 1 for even i, clamped to the level (J likewise)
 *   relax  `iters` Jacobi steps on the cells with n == 0: (((U + D) + L) + R) * 0.25, the
 *          neighbours index-clamped, every read from the previous iterate
 * Pull up to 1 x 1, then from the top down push and relax at EVERY level.  Finite cells come
 * out bit-identical; the output is finite everywhere unless the whole map is a hole, and
 * then it is the input bit for bit.  tests/test_fill_host.py restates this in numpy; the
 * kernels equal it bit for bit. */

/* Bytes of the workspace dm_fill_holes needs for M maps of H x W cells; 0 for a shape it does
 * not take (a count below 1, H W > 2^31 - 1, M > 65535, a side above 64 * 65535). */
size_t dm_fill_bytes(int32_t M, int32_t H, int32_t W);

/* d_out [M][H][W] receives the filled maps and may equal d_in (in place).  d_holes
 * ([M][H][W] uint8, may be NULL) receives 1 where the input cell was a hole, else 0.  d_work:
 * dm_fill_bytes(M, H, W) bytes, 16-byte aligned, contents arbitrary.  0 <= iters <= 4096
 * Jacobi steps per level.  DM_ERR_ARG for a null d_in / d_out / d_work, a count below 1 or
 * iters out of range; DM_ERR_UNSUPPORTED for the other shapes dm_fill_bytes refuses.
 * Validation precedes every HIP call. */
int dm_fill_holes(const double *d_in, int32_t M, int32_t H, int32_t W, int32_t iters,
                  double *d_out, uint8_t *d_holes, void *d_work, void *stream);

/* ---- Speckle filter (dm_speckle.hip) -----------------------------------------------------
 * Not in the reference.  The round-trip check keeps a mismatch when both directions agree on
 * the wrong place, and the fill and the sweeps below then smear that blob into its neighbours.
 * dm_filter_speckles removes small isolated segments of a map, as OpenCV's filterSpeckles
 * does, each of the M maps of d_in [M][H][W] on its own:
 *   finite   a cell that passes the range test made on the double; NaN and +-inf are holes
 *   joined   two finite 4-neighbours a, b with fabs(a - b) <= max_diff, in float64 without
 *            contraction (a difference that overflows to inf is joined only by max_diff = +inf)
 *   segment  a connected component of the join graph; its size is its cell count, its label
 *            the smallest linear index i W + j among its cells
 * Every cell of a segment with size <= max_size becomes NaN in d_out (the quiet NaN dm_stitch
 * writes); every other cell, input holes included, is copied bit for bit.  max_size = 0
 * removes nothing and still reports sizes and labels.  Labels and sizes are integers and do
 * not depend on the schedule: the outputs are bit-identical from run to run.
 * tests/test_speckle_host.py restates this in plain loops; the kernels equal it bit for bit. */

/* Bytes of the workspace dm_filter_speckles needs for M maps of H x W cells; 0 for a shape it
 * does not take (a count below 1, H W > 2^31 - 1: labels are int32, M > 65535, a side above
 * 64 * 65535). */
size_t dm_speckle_bytes(int32_t M, int32_t H, int32_t W);

/* d_out [M][H][W] may equal d_in (in place).  Optional outputs, each [M][H][W] and may be
 * NULL: d_removed (uint8) 1 where this call removed the cell, else 0 (input holes: 0); d_size
 * (uint32) the size of the cell's segment as found, 0 at input holes; d_label (int32) its
 * label, -1 at input holes.  d_work: dm_speckle_bytes(M, H, W) bytes, 16-byte aligned,
 * contents arbitrary.  DM_ERR_ARG for a null d_in / d_out / d_work, a count below 1,
 * max_size < 0, a negative or NaN max_diff (+inf is allowed); DM_ERR_UNSUPPORTED for the other
 * shapes dm_speckle_bytes refuses.  Validation precedes every HIP call; nothing is allocated,
 * nothing synchronises, all work goes on `stream`. */
int dm_filter_speckles(const double *d_in, int32_t M, int32_t H, int32_t W, int32_t max_size,
                       double max_diff, double *d_out, uint8_t *d_removed, uint32_t *d_size,
                       int32_t *d_label, void *d_work, void *stream);

/* ---- Joint bilateral filter (dm_bilateral.hip) -------------------------------------------
 * The live branch of the reference's optimize_looper.py (:76-77) is cv2.bilateralFilter on a
 * uint8 cast of the map.  dm_bilateral_filter is its float64, NaN-aware, guided form: it
 * smooths each of the M maps of d_in [M][H][W] on its own.  All arithmetic is float64 without
 * contraction, in the order written; exp is the pinned dm_exp (csrc/dm_exp.h).  One pass, with
 * input X and guide G:
 *   guide    d_guide NULL: the map guides itself, G is X (in a later pass that pass's input).
 *            Otherwise G is d_guide, [H][W] shared by all maps (guide_maps == 1) or [M][H][W]
 *            (guide_maps == M), float64, or uint8 with DM_BILAT_GUIDE_U8 (value (double)g);
 *            an external guide is the same in every pass.
 *   usable   a tap inside the map at which X and G are both finite (range test on the double;
 *            NaN and +-inf in the map are holes, as in dm_fill_holes)
 *   cell     G[i, j] not finite: the output is X[i, j] bit for bit.  X[i, j] a hole and
 *            DM_BILAT_FILL not set: likewise.  Otherwise num = 0, den = 0 and, dy = -r .. r
 *            outer, dx = -r .. r inner, both ascending, for each usable tap (i + dy, j + dx):
 *              c  = G[i, j] - G[tap];  wc = dm_exp(-(c * c) / den_color)
 *              ws = dm_exp(-(double)(dy*dy + dx*dx) / den_space)
 *              w  = ws * wc;  a tap with !(w > 0) is skipped
 *              num = num + w * X[tap];  den = den + w
 *            The output is num / den when den > 0, else X[i, j] bit for bit.  A finite centre
 *            has den >= 1: its own tap weighs exactly 1.
 *   FILL     DM_BILAT_FILL (needs an external guide): a hole whose window holds a usable tap
 *            is filled from those taps.
 * `iters` passes, pass k + 1 reading pass k's output.  It follows that without FILL a hole
 * stays bit-identical, that a map that is all holes comes out as it went in, that a finite
 * cell comes out finite as long as no w * X overflows, and that the outputs are bit-identical
 * from run to run (a thread sums its cell's window sequentially; no atomics).
 * den_color, den_space: 2.0 * sigma**2 as the caller's Python evaluates it (dm_make_weight's
 * convention); both > 0, +inf allowed (a flat weight).
 * tests/test_bilateral_host.py restates this in plain loops; the kernel equals it bit for
 * bit, and its uint8-guide path (a 256-entry table of wc) equals its float64-guide path. */
enum { DM_BILAT_FILL = 1, DM_BILAT_GUIDE_U8 = 2 };

/* Bytes of the workspace dm_bilateral_filter needs for M maps of H x W cells; 0 for a shape it
 * does not take (dm_fill_bytes' limits: a count below 1, H W > 2^31 - 1, M > 65535, a side
 * above 64 * 65535). */
size_t dm_bilateral_bytes(int32_t M, int32_t H, int32_t W);

/* d_out [M][H][W] may equal d_in (in place).  d_filled ([M][H][W] uint8, may be NULL) receives
 * 1 where d_in was a hole and d_out is finite, else 0.  d_work: dm_bilateral_bytes(M, H, W)
 * bytes, 16-byte aligned, contents arbitrary.  1 <= radius <= 15, 1 <= iters <= 64.
 * DM_ERR_ARG for a null d_in / d_out / d_work, a count below 1, radius or iters out of range,
 * a den_* that is not > 0 (NaN included), unknown flag bits, guide_maps not 1 or M when a
 * guide is given, DM_BILAT_FILL or DM_BILAT_GUIDE_U8 without a guide; DM_ERR_UNSUPPORTED for
 * the other shapes dm_bilateral_bytes refuses.  Validation precedes every HIP call; nothing is
 * allocated, nothing synchronises, all work goes on `stream`. */
int dm_bilateral_filter(const double *d_in, const void *d_guide /* may be NULL */, int32_t guide_maps,
                        int32_t M, int32_t H, int32_t W, int32_t radius, double den_color, double den_space,
                        int32_t iters, int32_t flags, double *d_out, uint8_t *d_filled /* may be NULL */,
                        void *d_work, void *stream);

/* ---- Weighted median filter (dm_median.hip) ----------------------------------------------
 * Not in the reference, whose filtering_mode = 'median' (Matching._filter) works inside one
 * tile, on integer correspondences, before the stitch.  dm_median_filter is the impulse filter
 * of the stitched map: dm_filter_speckles only turns outliers into holes, and only those that
 * form a segment of their own, and dm_bilateral_filter spreads a wrong cell over its
 * neighbours.  It filters each of the M maps of d_in [M][H][W] on its own.  One pass, with
 * input X:
 *   key      the order-preserving 64-bit integer of a double: with the sign bit set all bits
 *            are flipped, otherwise the sign bit is set.  -0.0 sorts before +0.0 and equal keys
 *            mean equal bits; "smaller" and "larger" below are by key
 *   finite   a cell that passes the range test made on the double; NaN and +-inf are holes, as
 *            in dm_fill_holes
 *   weights  d_weight NULL: the unweighted form.  Otherwise float64, [H][W] shared by all maps
 *            (weight_maps == 1) or [M][H][W] (weight_maps == M), the same in every pass
 *   usable   a tap inside the map at which X is finite and, with weights, the weight w
 *            satisfies w > 0 && w < +inf (a NaN weight is not usable)
 *   cell     X[i, j] a hole and DM_MEDIAN_FILL not set: the output is X[i, j] bit for bit.
 *            Otherwise take the usable taps of the (2r + 1)^2 window clipped to the map in
 *            window order, dy = -r .. r outer, dx = -r .. r inner, both ascending; n is their
 *            number.  n < min_count: the output is X[i, j] bit for bit.  Else
 *              unweighted  the tap value of rank (n - 1) / 2 (0-based, ascending): the lower
 *                          median
 *              weighted    T = the float64 sum of the usable taps' weights in window order,
 *                          from 0.0, one rounding per addition, no contraction; S(v) = the sum
 *                          formed the same way, in the same order, over the usable taps whose
 *                          key <= key(v); the output is the smallest tap value v with
 *                          S(v) >= 0.5 * T
 *            S is monotone in v (floating-point addition is monotone, and a superset of
 *            non-negative terms added in the same order never sums lower) and S(max) = T, so
 *            the smallest such v exists and a bisection over keys finds it.  With all weights
 *            1.0 the weighted rule equals the unweighted one bit for bit.
 *   FILL     DM_MEDIAN_FILL: a hole with n >= min_count usable taps receives the median.
 * `iters` passes, pass k + 1 reading pass k's output.  It follows that every finite output is
 * bit-identical to some input cell of its window, that without FILL a hole stays
 * bit-identical, that a map that is all holes comes out as it went in, and that the outputs
 * are bit-identical from run to run (a thread selects its own cell's value; no atomics).
 * tests/test_median_host.py restates this in plain loops; the kernel equals it bit for bit. */
enum { DM_MEDIAN_FILL = 1 };

/* Bytes of the workspace dm_median_filter needs for M maps of H x W cells; 0 for a shape it
 * does not take (dm_fill_bytes' limits: a count below 1, H W > 2^31 - 1, M > 65535, a side
 * above 64 * 65535). */
size_t dm_median_bytes(int32_t M, int32_t H, int32_t W);

/* d_out [M][H][W] may equal d_in (in place).  d_changed ([M][H][W] uint8, may be NULL)
 * receives 1 where the output's bits differ from d_in's, else 0.  d_work:
 * dm_median_bytes(M, H, W) bytes, 16-byte aligned, contents arbitrary.  1 <= radius <= 7,
 * 1 <= iters <= 64, 1 <= min_count <= (2 radius + 1)^2.  DM_ERR_ARG for a null d_in / d_out /
 * d_work, a count below 1, radius, iters or min_count out of range, unknown flag bits,
 * weight_maps not 1 or M when weights are given; DM_ERR_UNSUPPORTED for the other shapes
 * dm_median_bytes refuses.  Validation precedes every HIP call; nothing is allocated, nothing
 * synchronises, all work goes on `stream`. */
int dm_median_filter(const double *d_in, const double *d_weight /* may be NULL */, int32_t weight_maps,
                     int32_t M, int32_t H, int32_t W, int32_t radius, int32_t min_count, int32_t iters,
                     int32_t flags, double *d_out, uint8_t *d_changed /* may be NULL */,
                     void *d_work, void *stream);

/* ---- Photo-consistency score (dm_photo.hip) -----------------------------------------------
 * Not in the reference.  out_map is the matcher's score of the correspondence it found: its
 * level 0 is normalised per patch, and the median, the fill and the smoothing move cells without
 * updating it.  dm_photo_score judges any map, however it was produced: it resamples img2 at
 * the position the map claims for a cell and correlates it with img1 around the cell (zero-mean
 * normalised cross-correlation, in [-1, 1]).
 *   images   img1, img2: uint8 [Hi][Wi], rows stride1 / stride2 bytes apart (>= Wi)
 *   planes   d_row, d_col: float64 [H][W], the 'elevation2' and 'elevation' maps: elevation =
 *            j - match_col, elevation2 = i - match_row (Calc_difference.cal_map), so the match of
 *            a cell lies at its own position minus the disparity
 *   offsets  map cell (y, x) is image pixel (cy, cx) = (y + oy, x + ox)
 *   window   radius r, 1 <= r <= 7, n = (2r + 1)^2
 * Per cell:
 *   1. d_row or d_col not finite (the range test on the double: NaN and +-inf fail): the cell
 *      is unscored and has no warped value.
 *   2. py = (double)cy - d_row, px = (double)cx - d_col.  The tests of 3 and 6 are made on py and
 *      px in double; only a position that passed them is converted: iy = floor(py), ix =
 *      floor(px), fy = py - iy, fx = px - ix (exact, in [0, 1)).
 *   3. The cell is unscored unless the img1 window, rows cy-r .. cy+r and columns cx-r .. cx+r,
 *      and the img2 patch, rows iy-r .. iy+r+1 and columns ix-r .. ix+r+1, lie inside the image:
 *      r <= py < Hi - r - 1 and r <= px < Wi - r - 1.  The extra row and column are required
 *      even when fy or fx is 0: one rule, no special case.
 *   4. A is the img1 window, P0, P1, P2, P3 the (2r+1)^2 windows of img2 whose top-left corners
 *      are (iy-r, ix-r) + (0,0), (0,1), (1,0), (1,1).  As exact integers (sums over the window's
 *      n taps):
 *        sa = sum A, saa = sum A^2, S_k = sum P_k,
 *        CA_k = n sum(A P_k) - sa S_k,   CB_kl = n sum(P_k P_l) - S_k S_l (k <= l),
 *        VA = n saa - sa^2
 *      (n sum(P_k P_l) reaches 3.29e9 at r = 7: 64-bit arithmetic).  Each is below 2^53 in
 *      magnitude and converts to double exactly.
 *   5. In float64, one rounding per operation, no contraction:
 *        w0 = (1-fy) * (1-fx), w1 = (1-fy) * fx, w2 = fy * (1-fx), w3 = fy * fx
 *        num = ((w0 CA_0 + w1 CA_1) + w2 CA_2) + w3 CA_3
 *        vb  = the sum, left to right, over k <= l (k outer, l inner: 00 01 02 03 11 12 13 22 23
 *              33) of (c * (w_k * w_l)) * CB_kl, c = 1 for k = l, else 2
 *        score = 0.0 unless VA > 0 and vb > 0; else t = num / sqrt(VA * vb), and the score is
 *                1.0 if t > 1, -1.0 if t < -1, else t
 *   6. warped (optional) = ((w0 q00 + w1 q01) + w2 q10) + w3 q11 with q the img2 pixels at
 *      (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1), whenever those four lie inside the image
 *      (0 <= py < Hi - 1 and 0 <= px < Wi - 1), whatever rule 3 says; else NaN.
 *   7. An unscored cell has the score NaN (0x7ff8000000000000).
 * Rejection (DM_PHOTO_REJECT, threshold min_score in [-1, 1]): in every one of the M planes of
 * d_maps [M][H][W] a cell whose score is not NaN and is below min_score becomes NaN
 * (0x7ff8000000000000); every other cell, the unscored ones included, keeps its bits.
 * d_rejected (uint8 [H][W]) receives 1 at exactly those cells, else 0.  A cell reads only its
 * own d_row / d_col and they are read before d_maps is written, so d_row and d_col may be
 * planes of d_maps.
 * It follows that with integer disparities and identical windows the score is exactly 1.0
 * (sqrt(x * x) = x), that a flat window on either side gives exactly 0.0, and that the result
 * does not depend on the order of summation: every sum is an integer.
 * tests/test_photo_host.py restates this in plain loops; the kernel equals it bit for bit. */
enum { DM_PHOTO_REJECT = 1 };

/* Bytes of the workspace dm_photo_score asks for (it needs none: a constant 16); 0 for a shape
 * it does not take (dm_median_bytes' limits). */
size_t dm_photo_bytes(int32_t M, int32_t H, int32_t W);

/* d_score, d_warped (float64 [H][W]) and d_rejected may be NULL.  Without DM_PHOTO_REJECT
 * d_maps, M and min_score are not read, d_rejected must be NULL and one of d_score / d_warped
 * must be given.  d_work: dm_photo_bytes(M, H, W) bytes, not NULL.  DM_ERR_ARG for a null
 * image / plane / workspace, a side below 1, a stride below Wi, an offset outside
 * [-2^30, 2^30], a radius outside [1, 7], unknown flag bits, with DM_PHOTO_REJECT a null
 * d_maps, M < 1 or a min_score outside [-1, 1] (NaN included); DM_ERR_UNSUPPORTED for the
 * other shapes dm_photo_bytes refuses.  Validation precedes every HIP call; nothing is
 * allocated, nothing synchronises, one launch on `stream`. */
int dm_photo_score(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2,
                   int32_t Hi, int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W,
                   int32_t oy, int32_t ox, int32_t radius, int32_t flags, double min_score,
                   double *d_maps /* may be NULL */, int32_t M, double *d_score /* may be NULL */,
                   double *d_warped /* may be NULL */, uint8_t *d_rejected /* may be NULL */,
                   void *d_work, void *stream);

/* ---- Local re-matching of a disparity map (dm_photo_refine.hip) -----------------------------
 * Not in the reference.  Rejection turns a wrong cell into a hole and the fill puts a guess
 * there; dm_photo_refine measures a cell again: it scores the (2s+1)^2 integer neighbours of
 * the position the map claims with dm_photo_score's correlation and moves the cell to the best
 * one.  Images, planes, offsets and the radius r in [1, 7] are dm_photo_score's; `search` is s in
 * [1, 3], min_gain in [0, 2].  Per cell (y, x), (cy, cx) = (y + oy, x + ox):
 *   1. The cell is skipped if d_mask is given and 0 at the cell, if d_row or d_col is not finite
 *      (the range test on the double), if the img1 window, rows cy-r .. cy+r and columns
 *      cx-r .. cx+r, leaves the image, or if py = (double)cy - d_row or px = (double)cx - d_col
 *      lies outside [-2^30, 2^30] (tested on the double, before any conversion).  A skipped cell
 *      copies both planes bit for bit, NaN payloads and -0.0 included; its score is NaN
 *      (0x7ff8000000000000), its shift (0, 0).
 *   2. iy = floor(py), ix = floor(px), fy = py - iy, fx = px - ix and w0 .. w3 as in
 *      dm_photo_score's rules 2 and 5.  A candidate is (dy, dx), integers in [-s, s]^2; it is
 *      scored iff r <= iy+dy <= Hi-r-2 and r <= ix+dx <= Wi-r-2.  Its score is dm_photo_score's
 *      rules 4 and 5 with the four img2 windows whose top-left corners are (iy+dy-r, ix+dx-r) +
 *      (0,0), (0,1), (1,0), (1,1) and the same weights: exact integer sums, the float64 tail in
 *      the same order, clamped to [-1, 1].  So candidate (0, 0) is scored exactly where
 *      dm_photo_score gives a score that is not NaN, and has that score's bits.
 *   3. The winner is the scored candidate with the highest score; ties go to the smallest
 *      dy^2 + dx^2, then the smaller dy, then the smaller dx.  If the centre (0, 0) is scored and
 *      `winner > centre + min_gain` (one float64 add, one compare) is false, the centre wins.  If
 *      no candidate is scored the cell is skipped as in 1.
 *   4. The centre wins: both planes are copied bit for bit, the score is the centre's, the shift
 *      (0, 0).  A map that is already locally best comes out unchanged to the bit.
 *   5. Another candidate wins, with score s0: ty = tx = 0.0.  With DM_REFINE_SUBPIX, per axis, if
 *      both neighbours of the winner along the axis lie in [-s, s] and are scored, with scores sm
 *      (at -1) and sp (at +1): den = (sm + sp) - 2.0 * s0, and if den < 0, t = (0.5 * (sm - sp)) /
 *      den, clamped to [-0.5, 0.5].  out_row = d_row - ((double)dy + ty), out_col = d_col -
 *      ((double)dx + tx).  The score is s0, the shift (dy, dx).
 *   6. A cell reads only its own d_row and d_col, before it writes: d_out_row and d_out_col may
 *      alias d_row and d_col.
 * tests/test_refine_host.py restates this in plain loops; the kernel equals it bit for bit. */
enum { DM_REFINE_SUBPIX = 1 };

/* Bytes of the workspace dm_photo_refine asks for (a constant 16: the kernel keeps everything on
 * chip); 0 for a shape it does not take: dm_photo_bytes' limits on H, W, Hi or Wi above 2^30, a
 * radius outside [1, 7] or a search outside [1, 3]. */
size_t dm_photo_refine_bytes(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t search);

/* d_mask (uint8 [H][W]), d_score (float64 [H][W]) and d_shift (int8 [2][H][W]: dy, then dx) may
 * be NULL.  d_work: dm_photo_refine_bytes(...) bytes, not NULL.  DM_ERR_ARG for a null image /
 * plane / output / workspace, a side below 1, a stride below Wi, an offset outside [-2^30, 2^30],
 * a radius outside [1, 7], a search outside [1, 3], a min_gain outside [0, 2] (NaN included),
 * unknown flag bits; DM_ERR_UNSUPPORTED for the other shapes dm_photo_refine_bytes refuses.
 * Validation precedes every HIP call; nothing is allocated, nothing synchronises, one launch on
 * `stream`; the result is the same from run to run. */
int dm_photo_refine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2,
                    int32_t Hi, int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W,
                    int32_t oy, int32_t ox, int32_t radius, int32_t search, double min_gain, int32_t flags,
                    const uint8_t *d_mask /* may be NULL */, double *d_out_row, double *d_out_col,
                    double *d_score /* may be NULL */, int8_t *d_shift /* may be NULL */,
                    void *d_work, void *stream);

/* ---- Least-squares sub-pixel matching of a disparity map (dm_lsm.hip) -----------------------
 * Not in the reference.  Every other stage moves a cell on the integer grid or interpolates it;
 * dm_lsm_refine measures the sub-pixel part: least-squares matching (Gruen 1985; the
 * Lucas-Kanade step) linearises img1 around the cell's window and solves, `iters` times, for the
 * shift that best explains the window by img2 resampled at the current position, gain and offset
 * left free.  Images, planes, offsets and the radius r in [1, 7] are dm_photo_score's; iters in
 * [1, 8], max_move a real in (0, 2].  cy, cx, py, px, iy, ix, fy, fx, A, P0..P3, n, sa, saa, S_k,
 * CA_k, CB_kl, VA, w0..w3, num, vb and "the score at a position" are dm_photo_score's rules 2-5
 * (rule 5 operation for operation); float64 throughout, one rounding per operation, no
 * contraction.  Per cell (y, x):
 *   1. The cell is skipped if d_mask is given and 0 at the cell, if d_row or d_col is not finite
 *      (dm_photo_score's rule 1), or if the img1 window with a one-pixel halo leaves the image:
 *      not (r+1 <= cy <= Hi-r-2 and r+1 <= cx <= Wi-r-2).  A skipped cell has status 0, the score
 *      NaN (0x7ff8000000000000), and copies both planes bit for bit.
 *   2. Once per cell, as exact integers over the window's taps (i, j): Gx(i,j) = A(i,j+1) -
 *      A(i,j-1), Gy(i,j) = A(i+1,j) - A(i-1,j) (doubled central differences, read from the halo),
 *        gx = sum Gx, gy = sum Gy,
 *        Hxx = n sum(Gx^2) - gx^2, Hyy = n sum(Gy^2) - gy^2, Hxy = n sum(Gx Gy) - gx gy,
 *        RAx = n sum(Gx A) - gx sa, RAy = n sum(Gy A) - gy sa.
 *      Each is below 2^53 in magnitude and converts to double exactly.  D = Hxx * Hyy - Hxy * Hxy
 *      in double (the products exceed int64 at r = 7).  Unless D > 0: status -1, the score NaN,
 *      the input is kept.
 *   3. (py0, px0) = ((double)cy - d_row, (double)cx - d_col).  If it fails dm_photo_score's rule
 *      3 (r <= py0 < Hi-r-1 and r <= px0 < Wi-r-1, tested on the double): status -2, the score
 *      NaN, the input is kept.  Else s0 is the score at (py0, px0).
 *   4. Step t = 1 .. iters from the current (py, px), which starts at (py0, px0): with the integer
 *      sums of dm_photo_score's rule 4 at this position and, for k = 0..3,
 *        GX_k = n sum(Gx P_k) - gx S_k,   GY_k = n sum(Gy P_k) - gy S_k
 *      (exact, converted to double), num and vb as in rule 5 there.  Unless vb > 0: status -1, the
 *      input is kept.  Else
 *        gbx = ((w0 GX_0 + w1 GX_1) + w2 GX_2) + w3 GX_3,   gby likewise with GY_k
 *        alpha = num / vb
 *        bx = RAx - alpha * gbx,   by = RAy - alpha * gby
 *        ux = ((Hyy * bx) - (Hxy * by)) / D,   uy = ((Hxx * by) - (Hxy * bx)) / D
 *        px = px + 2.0 * ux,   py = py + 2.0 * uy
 *      Unless |py - py0| <= max_move and |px - px0| <= max_move and the new position passes rule
 *      3 of dm_photo_score (a NaN fails): status -2, the input is kept.
 *   5. s1 is the score at the final position.  s1 > s0: the cell is accepted, status = iters,
 *      out_row = (double)cy - py, out_col = (double)cx - px, the score is s1.  Else status -3, the
 *      input bits are kept, the score is s0.  A cell that ended with -1 or -2 in rule 4 has the
 *      score s0.
 *   6. A cell reads only its own d_row and d_col, before it writes: d_out_row and d_out_col may
 *      alias d_row and d_col.  The result depends on nothing but the cell.
 * The factor 2.0 undoes the doubling of the differences: with g = G / 2 the normal equations are
 * (H / 4) u' = b / 2.  It follows that a cell on identical windows at an integer disparity has
 * alpha = 1.0, bx = by = 0.0 and status -3 (it never moves), that an accepted cell scores
 * strictly above dm_photo_score of the input, and that an unaccepted scored cell reports
 * dm_photo_score's bits.  tests/test_lsm_host.py restates this in plain loops; the kernel equals
 * it bit for bit. */

/* Bytes of the workspace dm_lsm_refine asks for (a constant 16: the kernel keeps everything on
 * chip); 0 for a shape it does not take: dm_photo_bytes' limits on H, W, Hi or Wi above 2^30, a
 * radius outside [1, 7] or iters outside [1, 8]. */
size_t dm_lsm_refine_bytes(int32_t Hi, int32_t Wi, int32_t H, int32_t W, int32_t radius, int32_t iters);

/* d_mask (uint8 [H][W]), d_score (float64 [H][W]) and d_status (int8 [H][W]) may be NULL.  d_work:
 * dm_lsm_refine_bytes(...) bytes, not NULL.  flags must be 0.  DM_ERR_ARG for a null image /
 * plane / output / workspace, a side below 1, a stride below Wi, an offset outside [-2^30, 2^30],
 * a radius outside [1, 7], iters outside [1, 8], a max_move outside (0, 2] (NaN included), a flag
 * bit; DM_ERR_UNSUPPORTED for the other shapes dm_lsm_refine_bytes refuses.  Validation precedes
 * every HIP call; nothing is allocated, nothing synchronises, one launch on `stream`; the result
 * is the same from run to run. */
int dm_lsm_refine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2,
                  int32_t Hi, int32_t Wi, const double *d_row, const double *d_col, int32_t H, int32_t W,
                  int32_t oy, int32_t ox, int32_t radius, int32_t iters, double max_move, int32_t flags,
                  const uint8_t *d_mask /* may be NULL */, double *d_out_row, double *d_out_col,
                  double *d_score /* may be NULL */, int8_t *d_status /* may be NULL */,
                  void *d_work, void *stream);

/* ---- Disparity priors: offset img2 crops for the unchanged solver (dm_prior.hip) --------------
 * Not in the reference, which cuts tile t at one origin o_t in img1 and img2: a cell whose match
 * lies outside its own tile of img2 cannot be found, and the share of correct cells falls like
 * 1 - |d| / S with the disparity d.  With an expected disparity q_t = (row, column) per tile, in
 * the units and sign of d_map ('elevation2', 'elevation': cell minus match), the img2 crop is cut
 * at o_t - q_t, which brings the disparity inside the tile back to about 0.  No kernel of the solve
 * changes: dm_pack_tiles copies the crop pairs into a fresh image pair, the existing entries solve
 * it at the grid's origins, dm_shift_matches moves the matches into the frame of img1's tile, so
 * that dm_cal_map, dm_stitch and dm_stitch_merge give global disparities (local + q').
 * dm_tile_prior takes the q_t from a map of the same pair, dm_downsample2 makes the
 * half-resolution pair such a map can be solved on.  tests/test_prior.py restates all four in
 * numpy; the kernels equal it bit for bit.  Nothing here allocates or synchronises.
 *
 * dm_downsample2: dst[y][x] = (s[2y][2x] + s[2y][2x+1] + s[2y+1][2x] + s[2y+1][2x+1] + 2) >> 2 for
 * the (H / 2) x (W / 2) destination (integer division: an odd last row or column is dropped).
 * Strides in bytes.  DM_ERR_ARG for a null pointer, H or W below 2, a stride below its width. */
int dm_downsample2(const uint8_t *d_src, int64_t stride, int32_t H, int32_t W, uint8_t *d_dst,
                   int64_t dst_stride, void *stream);

/* d_row, d_col: float64 [Hc][Wc], the 'elevation2' and 'elevation' planes of a map whose cell
 * (y, x) sits at pixel (y + e, x + e) of an image `scale` (1 or 2) times smaller than the one the
 * T tiles (d_origins int32 [T][2], h0 x w0 cells) are cut from.  Tile t covers image rows first =
 * o_y + e .. last = o_y + e + h0 - 1; its footprint rows are first / scale - e .. last / scale - e
 * (integer division), each end clamped into [0, Hc - 1], columns alike -- a footprint wholly
 * outside the map becomes its nearest edge row or column.  Over the footprint cells where BOTH
 * planes are finite (the range test on the double), n of them, the lower median of each plane is
 * its element (n - 1) / 2 in the order of the order-preserving key of the double
 * (dm_median_filter's); q = rint(scale * median), ties to even, clamped to [-2^30, 2^30], as int32.
 * d_valid[t] = 1 and d_q[t] = (q_row, q_col) for such a tile.  A tile with n = 0 has d_valid[t] = 0
 * and takes, per component, the lower median of the q of the tiles with d_valid = 1, or 0 if there
 * is none.  One workgroup per tile plus one small launch for the fallback; integer counting only,
 * the result is the same from run to run.  DM_ERR_ARG for a null pointer, a side below 1, Hc Wc or
 * h0 w0 above 2^31 - 1, h0 / w0 / e above 65536, e below 0, another scale. */
int dm_tile_prior(const double *d_row, const double *d_col, int32_t Hc, int32_t Wc, const int32_t *d_origins,
                  int32_t T, int32_t h0, int32_t w0, int32_t e, int32_t scale, int32_t *d_q, uint8_t *d_valid,
                  void *stream);

/* HOST function (no device work): the packed pair of T tiles.  A crop has ch = h0 + ws - 1 rows and
 * cw = w0 + ws - 1 columns; crop t sits at row (t / grid_cols) * ch, column (t % grid_cols) * cw of a
 * uint8 image of *Hp rows and *Wp columns, *Wp a multiple of 16 (the pitch of the packed images:
 * they are contiguous).  DM_ERR_UNSUPPORTED for a batch it does not take (a side below 1, a crop
 * side above 65536, a packed side above 2^30). */
int dm_pack_plan(int32_t T, int32_t h0, int32_t w0, int32_t ws, int32_t *grid_cols, int32_t *Hp, int32_t *Wp);

/* Crop t of img1 is cut at o_t (d_origins, int32 [T][2]), crop t of img2 at o_t - q_t (d_prior,
 * int32 [T][2]) clamped per axis into [0, H - ch] / [0, W - cw], so every packed crop pixel is a
 * real pixel; d_q_eff[t] = o_t - the clamped origin is the prior that took effect.  The crops go
 * to dm_pack_plan's places in d_pack1 / d_pack2 (contiguous *Hp x *Wp, 16-byte aligned); the cells
 * of the grid beyond T and the columns beyond grid_cols * cw are 0.  d_pack_origins (int32 [T][2])
 * receives the crops' places: the packed pair with these origins is a dm_tiles batch whose tile t
 * has exactly the two crops above.  The o_t must lie inside the image (the caller's check, as for
 * dm_tiles; the kernel clamps them like the img2 origins, so it never reads outside).  DM_ERR_ARG
 * for a null pointer, an image smaller than a crop or above 2^30 a side, a stride below W, a
 * packed image that is not 16-byte aligned; DM_ERR_UNSUPPORTED as dm_pack_plan. */
int dm_pack_tiles(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t H,
                  int32_t W, const int32_t *d_origins, const int32_t *d_prior, int32_t T, int32_t h0, int32_t w0,
                  int32_t ws, uint8_t *d_pack1, uint8_t *d_pack2, int32_t *d_pack_origins, int32_t *d_q_eff,
                  void *stream);

/* In place on dm_match's output, float64 [T][3][h0][w0]: map[t][0] -= q_eff[t][0], map[t][1] -=
 * q_eff[t][1] (one float64 subtraction of the converted integer: NaN stays NaN), the score row is
 * not touched.  A match position of the packed solve, expressed in img2's offset crop, becomes a
 * position in the frame of img1's tile; it may lie outside [0, h0) x [0, w0). */
int dm_shift_matches(double *d_match, const int32_t *d_q_eff, int32_t T, int32_t h0, int32_t w0, void *stream);

/* ----Gauss-Seidel post-processing (dm_postproc.hip) -------------
 * misc/optimize_loop.py (optimize_loop :15-37, image_threshold :40-44) and misc/opt_loop.py
 * (optimize_loop_bilateral_horizon :16-35, _vertical :39-58, make_weight :60-85).  Maps are
 * float64 row-major h x w; `size` = (s0, s1) <= (h, w) bounds the sweeps as in the
 * reference; excl = `exclusion` (e).  A sweep updates the (s0-2e-1) x (s1-2e-1) cells of
 * its fixed reference order in place; here it runs as dependency levels (dm_gs_schedule)
 * and gives the sequential loops' float64 results bit for bit. */
enum dm_gs_kind {
    DM_GS_FWD4 = 0,  /* optimize_loop forward sweep, 4-neighbour (optimize_loop.py:18-25)          */
    DM_GS_BWD4 = 1,  /* optimize_loop backward sweep, with the reference's row alternation (:27-36) */
    DM_GS_BILAT = 2  /* optimize_loop_bilateral_*, (2e+1)^2 window (opt_loop.py:23-35)              */
};

/* HOST function (no device work): the dependency-level schedule of one sweep.  n =
 * max(0, s0-2e-1) * max(0, s1-2e-1) updates; order[n] receives the update sequence indices
 * grouped by level, level_off[n_levels + 1] (capacity n + 1) the level boundaries.  An
 * update's level exceeds those of the last writers of every cell it reads and of every
 * reader of its own cell since that cell's last write, so one level's updates are
 * independent and the sequential order's values are reproduced exactly. */
int dm_gs_schedule(int32_t kind, int32_t h, int32_t w, int32_t s0, int32_t s1, int32_t excl,
                   int32_t *order, int32_t *level_off, int32_t *n_levels);

/* image_threshold (optimize_loop.py:40-44): out = min(max(in, lo), hi) as two np.where
 * (NaN passes through).  In place allowed. */
int dm_image_threshold(const double *d_in, size_t n, double lo, double hi, double *d_out,
                       void *stream);

/* optimize_loop (optimize_loop.py:15-37) on an already thresholded map d_img (in place):
 * forward sweep then backward sweep of d = (-a x + alpha (L+R+U+D)) / (-a + 4 alpha),
 * a = coefficient[i, j] (d_coef hc x wc).  Schedules from dm_gs_schedule (DM_GS_FWD4,
 * DM_GS_BWD4) in device memory.  d_diff: n float64 scratch; *d_error = the backward
 * sweep's sum of |x - d| in sequence order. */
int dm_optimize_loop(double *d_img, const double *d_coef, int32_t hc, int32_t wc, int32_t h,
                     int32_t w, int32_t s0, int32_t s1, int32_t excl, double alpha,
                     const int32_t *d_fwd_order, const int32_t *d_fwd_off, int32_t fwd_levels,
                     const int32_t *d_bwd_order, const int32_t *d_bwd_off, int32_t bwd_levels,
                     double *d_diff, double *d_error, void *stream);

/* make_weight (opt_loop.py:60-85): d_gauss[(2e+1)^2] = exp(-(dy^2+dx^2) / den_space),
 * d_color[s0-e][s1-e][2e+1][2e+1] = exp(-(c^2) / den_color) with c = guide[i,j] -
 * guide[i+dy, j+dx] on the filled cells, 0 elsewhere.  den_* = 2.0 * sigma[k]**2 as the
 * caller's Python evaluates it.  exp is the pinned dm_exp (csrc/dm_exp.h). */
int dm_make_weight(const double *d_guide, int32_t h, int32_t w, int32_t s0, int32_t s1,
                   int32_t excl, double den_color, double den_space, double *d_gauss,
                   double *d_color, void *stream);

/* optimize_loop_bilateral_horizon (vertical = 0) / _vertical (1) (opt_loop.py:16-58):
 * one sweep of d = (-a b + sum(g cw sub)) / (-a + sum(g cw)) in place on d_img, weights
 * from dm_make_weight, coefficients coefficient[e, e] and [e, e+-1] / [e+-1, e] of d_coef
 * (hc x wc), numpy's pairwise sum order.  Schedule: dm_gs_schedule(DM_GS_BILAT).
 * *d_error = sum of |x - d| in sequence order; d_diff: n float64 scratch. */
int dm_opt_loop_bilateral(double *d_img, const double *d_color, const double *d_gauss,
                          const double *d_coef, int32_t hc, int32_t wc, int32_t h, int32_t w,
                          int32_t s0, int32_t s1, int32_t excl, int32_t vertical,
                          const int32_t *d_order, const int32_t *d_off, int32_t n_levels,
                          double *d_diff, double *d_error, void *stream);

/* Sum of d_v[0..n) in sequence order, the float64 loop `error += v` of
 * misc/optimize_loop.py:34 / misc/opt_loop.py:33 bit for bit, for terms >= 0 (NaN and inf
 * propagate as in the loop).  Computed as exact integer prefix sums between the steps where
 * the running sum climbs a binade or a tie occurs (dm_postproc.hip, k_seq_sum_seg).  *d_out
 * (device) receives the sum; n == 0 gives +0.  The post-processing entries use it for their
 * error sums. */
int dm_seq_sum(const double *d_v, int64_t n, double *d_out, void *stream);

/* The compile-time tunables this library was built with ("C2_NB=4 C3_NB=2 ..."; see
 * dm_kernels.hip: DM_C*_NB, DM_C3_MINW, DM_VL_*), which decide the kernel instance each shape
 * launches -- tools/kernel_hash.py derives the profiled instances' symbols from it. */
const char *dm_build_config(void);

/* Human-readable description of the last failure on this thread. */
const char *dm_last_error(void);

/* ABI version (major * 100 + minor): 110 (1.1 adds dm_corr_level12, 1.2 the fp16 volume
 * dm_corr_volume_f16 / dm_rectify_f16, 1.3 the Gauss-Seidel post-processing, 1.4 a larger
 * stats workspace: a second window-operand region for the volume kernels, window stats
 * carried inside the operand tiles, 1.5 dm_corr_volume_ex, 1.6 dm_pow14_variant and the
 * 4-tile column groups of dm_corr_stats' window operands at S = 128 / 256, 1.7 dm_seq_sum,
 * 1.8 dm_subpix_map, 1.9 dm_subpix_map_tiles and the row-pair strips of dm_corr_stats'
 * workspace for the level kernel's min / max sweep, 1.10 the DM_POW_Q4G / DM_POW_KG forms of
 * dm_pow14_variant; those two forms went again with the pruned level kernel they served, the
 * values 4 and 5 now fail with DM_ERR_ARG like any unknown variant, and the version stays 110).
 * dm_fb_check, dm_stitch_fb, dm_fill_bytes, dm_fill_holes,
 * dm_stitch_merge, dm_speckle_bytes, dm_filter_speckles, dm_bilateral_bytes,
 * dm_bilateral_filter, dm_median_bytes, dm_median_filter, dm_debug_num_tile_f16,
 * dm_level_num_f16, dm_photo_bytes, dm_photo_score, dm_photo_refine_bytes, dm_photo_refine,
 * dm_lsm_refine_bytes, dm_lsm_refine, dm_downsample2, dm_tile_prior, dm_pack_plan, dm_pack_tiles and dm_shift_matches
 * are additive entries within 1.10:
 * no existing entry, struct or workspace changed, so the version stays 110. */
int dm_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* DMSTEREO_H */
