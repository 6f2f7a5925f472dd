// dm_fb.hip -- gfx950 kernels + C ABI of the forward-backward (left-right) consistency check.
//
// The reference has no such check: its one confidence signal is map[2], the sum of pyramid
// scores, and level 0 is min-max normalised per patch, so an occluded or textureless patch
// scores like a good one.  Here the pair is matched in both directions (img1 -> img2: F,
// img2 -> img1: B; both [T][3][h][w] as dm_match writes them, tile-local coordinates, the
// same crop window in both images as ImageCutSolver._cut_and_pool cuts it) and every cell
// is walked there and back:
//
//   r = F[t,0,i,j];  c = F[t,1,i,j]
//   qi = floor(r + 0.5);  qj = floor(c + 0.5)
//   if !(qi >= 0 && qi < h && qj >= 0 && qj < w)  err = NaN
//   else dr = B[t,0,qi,qj] - i;  dc = B[t,1,qi,qj] - j;  err = sqrt(dr*dr + dc*dc)
//   valid = err <= tol                                   (false for NaN)
//
// The range test is made on the doubles, before any conversion: NaN, +-inf, 1e300 and
// off-tile matches fail it and are never cast or used as an index.  All arithmetic is float64
// without contraction (-ffp-contract=off), so err equals a numpy evaluation bit for bit.
// k_fb_check writes err and the masked map per tile; k_stitch_fb is k_stitch
// (dm_kernels.hip) with the check evaluated at the tile cell each output pixel picks.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dm_fb_err.h"
#include "dm_host.h"      // dm_fail, DM_HIP_TRY

// masked may be NULL or alias fwd: a thread reads its own forward cell before it writes it,
// and no other thread reads that cell
__global__ void k_fb_check(const double *fwd, const double *bwd, int T, int h, int w, double tol, double *err,
                           double *masked)
{
    const size_t P = (size_t)h * w;
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)T * P) return;
    const size_t t = idx / P, l = idx % P;
    const int i = (int)(l / w), j = (int)(l % w);
    const double *f = fwd + t * 3 * P;
    const double r = f[l], c = f[P + l], s = f[2 * P + l];
    const double e = fb_err(f, bwd + t * 3 * P, P, h, w, i, j, l);
    err[idx] = e;
    if (masked) {
        const bool valid = e <= tol;
        double *m = masked + t * 3 * P;
        m[l] = valid ? r : NAN;
        m[P + l] = valid ? c : NAN;
        m[2 * P + l] = s;
    }
}

struct FbModes {
    int m[8];
};

// k_stitch's tile rule and cal_map expressions; every dmap mode is NaN where the cell fails
// the check, the score is map[2] unchanged
__global__ void k_stitch_fb(const double *fwd, const double *bwd, int n0, int n1, int h0, int w0, int s0, int s1,
                            FbModes modes, int nmodes, double tol, double *dmap, double *score, double *err,
                            int Hout, int Wout)
{
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t HW = (size_t)Hout * Wout;
    if (idx >= HW) return;
    const int y = (int)(idx / Wout), x = (int)(idx % Wout);
    const int i = min(y / s0, n0 - 1), j = min(x / s1, n1 - 1);
    const int ly = y - i * s0, lx = x - j * s1;
    if (ly >= h0 || lx >= w0) {
        for (int k = 0; k < nmodes; ++k) dmap[k * HW + idx] = NAN;
        score[idx] = NAN;
        err[idx] = NAN;
        return;
    }
    const size_t P = (size_t)h0 * w0, l = (size_t)ly * w0 + lx;
    const size_t tile = (size_t)j * n0 + i;
    const double *m = fwd + tile * 3 * P;
    const double e = fb_err(m, bwd + tile * 3 * P, P, h0, w0, ly, lx, l);
    const bool valid = e <= tol;
    for (int k = 0; k < nmodes; ++k) {
        double v;
        if (!valid) v = NAN;
        else if (modes.m[k] == DM_CAL_ELEVATION) v = (double)lx - m[P + l];
        else if (modes.m[k] == DM_CAL_ELEVATION2) v = (double)ly - m[l];
        else {
            const double a = (double)ly - m[l], b = (double)lx - m[P + l];
            v = sqrt(a * a + b * b);
        }
        dmap[k * HW + idx] = v;
    }
    score[idx] = m[2 * P + l];
    err[idx] = e;
}

static int check_tol(double tol)
{
    if (!(tol >= 0.0)) return dm_fail(DM_ERR_ARG, "tolerance must be >= 0 (got %g)", tol);
    return DM_OK;
}

// one thread per cell in blocks of 256: the block count must fit the grid's x dimension
static int fb_blocks(unsigned long long n, unsigned *blocks)
{
    const unsigned long long nb = (n + 255) / 256;
    if (nb > 0x7fffffffull) return dm_fail(DM_ERR_UNSUPPORTED, "map of %llu cells", n);
    *blocks = (unsigned)nb;
    return DM_OK;
}

extern "C" {

int dm_fb_check(const double *d_fwd, const double *d_bwd, int32_t T, int32_t h, int32_t w, double tol,
                double *d_err, double *d_masked, void *stream)
{
    if (!d_fwd || !d_bwd || !d_err) return dm_fail(DM_ERR_ARG, "null forward / backward / error pointer");
    if (T < 1 || h < 1 || w < 1) return dm_fail(DM_ERR_ARG, "bad fb_check shape T=%d h=%d w=%d", T, h, w);
    int rc = check_tol(tol);
    if (rc) return rc;
    unsigned nb;
    rc = fb_blocks((unsigned long long)T * (unsigned long long)h * (unsigned long long)w, &nb);
    if (rc) return rc;
    k_fb_check<<<nb, 256, 0, (hipStream_t)stream>>>(d_fwd, d_bwd, T, h, w, tol, d_err, d_masked);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

int dm_stitch_fb(const double *d_fwd, const double *d_bwd, int32_t n0, int32_t n1, int32_t h0, int32_t w0,
                 int32_t stride0, int32_t stride1, const int32_t *modes, int32_t nmodes, double tol,
                 double *d_dmap, double *d_score, double *d_err, void *stream)
{
    if (!d_fwd || !d_bwd || !d_dmap || !d_score || !d_err || n0 < 1 || n1 < 1 || h0 < 1 || w0 < 1 ||
        stride0 < 1 || stride1 < 1 || nmodes < 0 || nmodes > 8 || (nmodes && !modes))
        return dm_fail(DM_ERR_ARG, "bad stitch arguments");
    FbModes m;
    for (int k = 0; k < 8; ++k) m.m[k] = k < nmodes ? modes[k] : 0;
    for (int k = 0; k < nmodes; ++k)
        if (m.m[k] < 0 || m.m[k] > 2) return dm_fail(DM_ERR_ARG, "please input valid mode! (%d)", m.m[k]);
    int rc = check_tol(tol);
    if (rc) return rc;
    const long long Hout = (long long)stride0 * (n0 - 1) + h0, Wout = (long long)stride1 * (n1 - 1) + w0;
    if (Hout > 0x7fffffffLL || Wout > 0x7fffffffLL)
        return dm_fail(DM_ERR_UNSUPPORTED, "stitched map of %lld x %lld cells", Hout, Wout);
    unsigned nb;
    rc = fb_blocks((unsigned long long)Hout * (unsigned long long)Wout, &nb);
    if (rc) return rc;
    k_stitch_fb<<<nb, 256, 0, (hipStream_t)stream>>>(d_fwd, d_bwd, n0, n1, h0, w0, stride0, stride1, m, nmodes, tol,
                                                     d_dmap, d_score, d_err, (int)Hout, (int)Wout);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
