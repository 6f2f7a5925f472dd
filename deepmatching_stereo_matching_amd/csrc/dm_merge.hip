// dm_merge.hip -- gfx950 kernel + C ABI of the overlap-merging stitch (dm_stitch_merge).
//
// dm_stitch and dm_stitch_fb keep, of the tiles that cover an output pixel, the last one.  With
// overlapping tiles (stride S / 2: four solves per interior pixel) the other estimates are
// thrown away.  Here every covering tile is a candidate; include/dmstereo.h states the
// definition (candidates and their order, validity, weights, the four rules).  This file
// implements it with one thread per output pixel, x fastest, and without a per-thread
// candidate array:
//   pass 1   walks the candidates once (j outer, i inner, ascending): the 64-bit mask of the
//            valid ones (DM_MERGE_MAX_CAND = 64 bounds the candidates of a pixel), count,
//            spread, the rule's running values for LAST / CENTER / FEATHER, the minimum err.
//   median   ranks by re-enumeration: for each valid candidate its value is re-read and
//            compared with every other valid candidate's (the mask skips the invalid ones
//            without touching d_bwd again).  K^2 reads of cells this wave has just read.
// The modes select among three value expressions (k_stitch's), so the running values are kept
// per expression in named registers and picked per mode at the store: no array is indexed at
// run time, no scratch.  All arithmetic is float64 without contraction (-ffp-contract=off), in
// the order the header writes it.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dm_fb_err.h"
#include "dm_host.h"      // dm_fail, DM_HIP_TRY

struct MergeModes {
    int m[8];
};

// what the kernel needs besides the pointers
struct MergeGeom {
    int n0, n1, h0, w0, s0, s1, Hout, Wout;
    int nmodes, min_count;
    unsigned used; // bit e set: value expression e (a dm_cal_mode) is asked for by some mode
    double tol;
};

// k_stitch's three cal_map expressions of a cell (ly, lx) matched to (r, q)
__device__ __forceinline__ double mg_value(int e, int ly, int lx, double r, double q)
{
    if (e == DM_CAL_ELEVATION) return (double)lx - q;
    if (e == DM_CAL_ELEVATION2) return (double)ly - r;
    const double a = (double)ly - r, b = (double)lx - q;
    return sqrt(a * a + b * b);
}

__device__ __forceinline__ double mg_pick(int mode, double v0, double v1, double v2)
{
    return mode == DM_CAL_ELEVATION ? v0 : mode == DM_CAL_ELEVATION2 ? v1 : v2;
}

// the covering tiles of pixel (y, x): i in [i_lo, i_hi], j in [j_lo, j_hi] (empty: not covered)
struct MergeSpan {
    int i_lo, i_hi, j_lo, j_hi;
};

__device__ __forceinline__ MergeSpan mg_span(const MergeGeom &g, int y, int x)
{
    MergeSpan s;
    s.i_lo = y >= g.h0 ? (y - g.h0) / g.s0 + 1 : 0;
    s.i_hi = min(y / g.s0, g.n0 - 1);
    s.j_lo = x >= g.w0 ? (x - g.w0) / g.s1 + 1 : 0;
    s.j_hi = min(x / g.s1, g.n1 - 1);
    return s;
}

// Median of quantity `what` (0..2: a value expression, 3: the score) over the valid candidates
// (bit c of `mask`, m of them) by ranking: rank(c) = #{c' valid: v' < v or (v' == v and c' < c)}.
// The candidate that holds a wanted rank is the last one in order that has it; NaN when none
// has (only a NaN among the scores breaks the ranks' being a permutation).
__device__ __forceinline__ double mg_median(const double *fwd, const MergeGeom &g, const MergeSpan &sp, int y, int x,
                                            size_t P, unsigned long long mask, int m, int what)
{
    const int lo = (m - 1) >> 1, hi = m >> 1; // equal for odd m
    double a = NAN, b = NAN;
    int c = 0;
    for (int j = sp.j_lo; j <= sp.j_hi; ++j)
        for (int i = sp.i_lo; i <= sp.i_hi; ++i, ++c) {
            if (!((mask >> c) & 1ull)) continue;
            const int ly = y - i * g.s0, lx = x - j * g.s1;
            const double *f = fwd + ((size_t)j * g.n0 + i) * 3 * P + ((size_t)ly * g.w0 + lx);
            const double v = what == 3 ? f[2 * P] : mg_value(what, ly, lx, f[0], f[P]);
            int rank = 0, c2 = 0;
            for (int j2 = sp.j_lo; j2 <= sp.j_hi; ++j2)
                for (int i2 = sp.i_lo; i2 <= sp.i_hi; ++i2, ++c2) {
                    if (!((mask >> c2) & 1ull)) continue;
                    const int ly2 = y - i2 * g.s0, lx2 = x - j2 * g.s1;
                    const double *f2 = fwd + ((size_t)j2 * g.n0 + i2) * 3 * P + ((size_t)ly2 * g.w0 + lx2);
                    const double v2 = what == 3 ? f2[2 * P] : mg_value(what, ly2, lx2, f2[0], f2[P]);
                    rank += (v2 < v || (v2 == v && c2 < c)) ? 1 : 0;
                }
            if (rank == lo) a = v;
            if (rank == hi) b = v;
        }
    return (m & 1) ? a : (a + b) * 0.5;
}

template <int RULE, bool FB>
__global__ void __launch_bounds__(256)
k_stitch_merge(const double *__restrict__ fwd, const double *__restrict__ bwd, MergeGeom g, MergeModes modes,
               double *__restrict__ dmap, double *__restrict__ score, double *__restrict__ err,
               double *__restrict__ spread, uint8_t *__restrict__ count)
{
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t HW = (size_t)g.Hout * g.Wout;
    if (idx >= HW) return;
    const int y = (int)(idx / g.Wout), x = (int)(idx % g.Wout);
    const MergeSpan sp = mg_span(g, y, x);
    if (sp.i_lo > sp.i_hi || sp.j_lo > sp.j_hi) { // no tile covers
        for (int k = 0; k < g.nmodes; ++k) {
            dmap[k * HW + idx] = NAN;
            if (spread) spread[k * HW + idx] = NAN;
        }
        score[idx] = NAN;
        if (FB && err) err[idx] = NAN;
        if (count) count[idx] = 0;
        return;
    }
    const size_t P = (size_t)g.h0 * g.w0;
    const bool u0 = g.used & 1u, u1 = g.used & 2u, u2 = g.used & 4u;

    // ---- pass 1 ---------------------------------------------------------------------------
    unsigned long long mask = 0;
    int m = 0, c = 0;
    double mn0 = NAN, mn1 = NAN, mn2 = NAN, mx0 = NAN, mx1 = NAN, mx2 = NAN; // spread
    double o0 = NAN, o1 = NAN, o2 = NAN;                                     // the rule's values
    double osc = NAN, oer = NAN;                                             // its score and err
    double lsc = NAN, ler = NAN;                                             // last covering candidate's
    double den = 0.0, best = -1.0;
    if (RULE == DM_MERGE_FEATHER) o0 = o1 = o2 = osc = 0.0;
    for (int j = sp.j_lo; j <= sp.j_hi; ++j)
        for (int i = sp.i_lo; i <= sp.i_hi; ++i, ++c) {
            const int ly = y - i * g.s0, lx = x - j * g.s1;
            const size_t l = (size_t)ly * g.w0 + lx;
            const size_t tile = (size_t)j * g.n0 + i;
            const double *f = fwd + tile * 3 * P;
            const double r = f[l], q = f[P + l], s = f[2 * P + l];
            double e = NAN;
            bool valid = isfinite(r) && isfinite(q);
            if (FB) {
                e = fb_err(f, bwd + tile * 3 * P, P, g.h0, g.w0, ly, lx, l);
                valid = valid && e <= g.tol;
            }
            const double v0 = u0 ? mg_value(0, ly, lx, r, q) : NAN;
            const double v1 = u1 ? mg_value(1, ly, lx, r, q) : NAN;
            const double v2 = u2 ? mg_value(2, ly, lx, r, q) : NAN;
            lsc = s;
            ler = e;
            if (RULE == DM_MERGE_LAST) { // dm_stitch / dm_stitch_fb: the last covering tile, as it is
                const bool keep = !FB || e <= g.tol;
                o0 = keep ? v0 : NAN;
                o1 = keep ? v1 : NAN;
                o2 = keep ? v2 : NAN;
            }
            if (!valid) continue;
            mask |= 1ull << c;
            if (m == 0) {
                mn0 = mx0 = v0;
                mn1 = mx1 = v1;
                mn2 = mx2 = v2;
            } else {
                mn0 = v0 < mn0 ? v0 : mn0, mx0 = v0 > mx0 ? v0 : mx0;
                mn1 = v1 < mn1 ? v1 : mn1, mx1 = v1 > mx1 ? v1 : mx1;
                mn2 = v2 < mn2 ? v2 : mn2, mx2 = v2 > mx2 ? v2 : mx2;
            }
            if (RULE == DM_MERGE_CENTER) {
                const double gw = (double)min(ly + 1, g.h0 - ly) * (double)min(lx + 1, g.w0 - lx);
                if (gw >= best) best = gw, o0 = v0, o1 = v1, o2 = v2, osc = s, oer = e;
            } else if (RULE != DM_MERGE_LAST) {
                if (FB) oer = (m == 0 || e < oer) ? e : oer;
                if (RULE == DM_MERGE_FEATHER) {
                    const double gw = (double)min(ly + 1, g.h0 - ly) * (double)min(lx + 1, g.w0 - lx);
                    o0 = o0 + gw * v0;
                    o1 = o1 + gw * v1;
                    o2 = o2 + gw * v2;
                    osc = osc + gw * s;
                    den = den + gw;
                }
            }
            ++m;
        }

    // ---- the rule's result ----------------------------------------------------------------
    if (RULE == DM_MERGE_LAST) {
        osc = lsc;
        oer = ler;
    } else if (m == 0) { // covered, nothing valid: as dm_stitch_fb leaves such a pixel
        o0 = o1 = o2 = NAN;
        osc = lsc;
        oer = ler;
    } else {
        if (RULE == DM_MERGE_FEATHER) {
            o0 = o0 / den;
            o1 = o1 / den;
            o2 = o2 / den;
            osc = osc / den;
        }
        if (RULE == DM_MERGE_MEDIAN) {
            if (u0) o0 = mg_median(fwd, g, sp, y, x, P, mask, m, 0);
            if (u1) o1 = mg_median(fwd, g, sp, y, x, P, mask, m, 1);
            if (u2) o2 = mg_median(fwd, g, sp, y, x, P, mask, m, 2);
            osc = mg_median(fwd, g, sp, y, x, P, mask, m, 3);
        }
        if (m < g.min_count) o0 = o1 = o2 = NAN;
    }
    const double sp0 = mx0 - mn0, sp1 = mx1 - mn1, sp2 = mx2 - mn2; // NaN for m == 0
    for (int k = 0; k < g.nmodes; ++k) {
        const int mode = modes.m[k];
        dmap[k * HW + idx] = mg_pick(mode, o0, o1, o2);
        if (spread) spread[k * HW + idx] = mg_pick(mode, sp0, sp1, sp2);
    }
    score[idx] = osc;
    if (FB && err) err[idx] = oer;
    if (count) count[idx] = (uint8_t)m;
}

template <int RULE>
static void merge_launch(bool fb, unsigned nb, hipStream_t st, const double *fwd, const double *bwd,
                         const MergeGeom &g, const MergeModes &m, double *dmap, double *score, double *err,
                         double *spread, uint8_t *count)
{
    if (fb) k_stitch_merge<RULE, true><<<nb, 256, 0, st>>>(fwd, bwd, g, m, dmap, score, err, spread, count);
    else k_stitch_merge<RULE, false><<<nb, 256, 0, st>>>(fwd, bwd, g, m, dmap, score, err, spread, count);
}

// ceil(a / b) for a, b >= 1
static long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

extern "C" {

int dm_stitch_merge(const double *d_fwd, const double *d_bwd, int32_t n0, int32_t n1, int32_t h0, int32_t w0,
                    int32_t stride0, int32_t stride1, const int32_t *modes, int32_t nmodes, double tol,
                    int32_t rule, int32_t min_count, double *d_dmap, double *d_score, double *d_err,
                    double *d_spread, uint8_t *d_count, void *stream)
{
    if (!d_fwd || !d_dmap || !d_score || n0 < 1 || n1 < 1 || h0 < 1 || w0 < 1 || stride0 < 1 || stride1 < 1 ||
        nmodes < 0 || nmodes > 8 || (nmodes && !modes))
        return dm_fail(DM_ERR_ARG, "bad stitch arguments");
    MergeModes m;
    MergeGeom g;
    g.used = 0;
    for (int k = 0; k < 8; ++k) m.m[k] = k < nmodes ? modes[k] : 0;
    for (int k = 0; k < nmodes; ++k) {
        if (m.m[k] < 0 || m.m[k] > 2) return dm_fail(DM_ERR_ARG, "please input valid mode! (%d)", m.m[k]);
        g.used |= 1u << m.m[k];
    }
    if (rule < DM_MERGE_LAST || rule > DM_MERGE_MEDIAN)
        return dm_fail(DM_ERR_ARG, "merge rule must be 0..3 (got %d)", rule);
    if (min_count < 1 || min_count > 255)
        return dm_fail(DM_ERR_ARG, "min_count must be in [1, 255] (got %d)", min_count);
    if (rule == DM_MERGE_LAST && min_count != 1)
        return dm_fail(DM_ERR_ARG, "min_count must be 1 with the rule DM_MERGE_LAST (got %d)", min_count);
    if (d_err && !d_bwd) return dm_fail(DM_ERR_ARG, "an err output needs the backward tiles");
    if (d_bwd && !(tol >= 0.0)) return dm_fail(DM_ERR_ARG, "tolerance must be >= 0 (got %g)", tol);
    const long long Hout = (long long)stride0 * (n0 - 1) + h0, Wout = (long long)stride1 * (n1 - 1) + w0;
    if (Hout > 0x7fffffffLL || Wout > 0x7fffffffLL)
        return dm_fail(DM_ERR_UNSUPPORTED, "stitched map of %lld x %lld cells", Hout, Wout);
    const unsigned long long cells = (unsigned long long)Hout * (unsigned long long)Wout;
    const unsigned long long nb = (cells + 255) / 256;
    if (nb > 0x7fffffffull) return dm_fail(DM_ERR_UNSUPPORTED, "map of %llu cells", cells);
    const long long c0 = ceil_div(h0, stride0), c1 = ceil_div(w0, stride1);
    const long long cand = (n0 < c0 ? n0 : c0) * (n1 < c1 ? n1 : c1);
    if (cand > DM_MERGE_MAX_CAND)
        return dm_fail(DM_ERR_UNSUPPORTED, "up to %lld tiles cover one pixel, the merge takes %d", cand,
                     DM_MERGE_MAX_CAND);
    g.n0 = n0, g.n1 = n1, g.h0 = h0, g.w0 = w0, g.s0 = stride0, g.s1 = stride1;
    g.Hout = (int)Hout, g.Wout = (int)Wout;
    g.nmodes = nmodes, g.min_count = min_count;
    g.tol = d_bwd ? tol : 0.0;
    const hipStream_t st = (hipStream_t)stream;
    const bool fb = d_bwd != NULL;
    switch (rule) {
    case DM_MERGE_LAST:
        merge_launch<DM_MERGE_LAST>(fb, (unsigned)nb, st, d_fwd, d_bwd, g, m, d_dmap, d_score, d_err, d_spread, d_count);
        break;
    case DM_MERGE_CENTER:
        merge_launch<DM_MERGE_CENTER>(fb, (unsigned)nb, st, d_fwd, d_bwd, g, m, d_dmap, d_score, d_err, d_spread, d_count);
        break;
    case DM_MERGE_FEATHER:
        merge_launch<DM_MERGE_FEATHER>(fb, (unsigned)nb, st, d_fwd, d_bwd, g, m, d_dmap, d_score, d_err, d_spread, d_count);
        break;
    default:
        merge_launch<DM_MERGE_MEDIAN>(fb, (unsigned)nb, st, d_fwd, d_bwd, g, m, d_dmap, d_score, d_err, d_spread, d_count);
        break;
    }
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
