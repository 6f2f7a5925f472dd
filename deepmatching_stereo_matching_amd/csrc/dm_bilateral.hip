// dm_bilateral.hip -- gfx950 kernel + C ABI of the NaN-aware joint bilateral filter
// (dm_bilateral_filter, include/dmstereo.h).
//
// One pass, input X, guide G (G = X without an external guide).  A tap is usable when it lies
// inside the map and X and G are finite there (range test on the double).  A cell whose G is
// not finite, or whose X is a hole without DM_BILAT_FILL, is copied bit for bit.  Otherwise,
// dy = -r .. r outer, dx = -r .. r inner, over the usable taps, float64 without contraction:
//   c = G[i, j] - G[tap];  wc = dm_exp(-(c * c) / den_color)
//   ws = dm_exp(-(double)(dy dy + dx dx) / den_space);  w = ws * wc;  !(w > 0): skipped
//   num = num + w * X[tap];  den = den + w
// and the output is num / den when den > 0, else X[i, j] bit for bit.
// tests/test_bilateral_host.py restates this in plain loops (bilateral_restate); the kernel
// equals it bit for bit, whatever the tile side.
//
// k_bilat<GK>: one launch per pass, one workgroup of 256 threads per tile of T x T cells (T = 16
// or 32: bil_tile_shift), grid (tiles, M).  The tile with its halo of r cells is staged into
// LDS, and so is the spatial table ws[(2r+1)^2].  A thread owns the whole window of each of its
// T T / 256 cells and sums it sequentially in the order above: no atomics, no cross-lane
// reduction, so the result does not depend on T or on the schedule.
//   GK_U8    uint8 guide.  wc depends on |g0 - g1| only: a table of 512 float64 in LDS,
//            entries 0 .. 255 dm_exp(-(c c) / den_color), entries 256 .. 511 zero.  The guide
//            plane holds 511 at unusable taps (out of the map, X a hole), so their weight is
//            the table's +0, and the value plane holds +0 there: the inner loop is two table
//            reads, the value, two multiplies and two adds, without a test.  Adding w X = +-0
//            and w = +0 changes no bit: num and den start at +0, and a round-to-nearest sum
//            is -0 only when both terms are, so num is never -0 and x + (+-0) == x.  A usable
//            tap whose w underflows to 0 is "skipped" the same way.
//   GK_F64   float64 guide: the guide plane holds NaN at unusable taps, c and w are then NaN
//            and the tap fails w > 0.  dm_exp per tap.
//   GK_SELF  the map guides itself: one plane.  A hole tap gives c = NaN or +-inf, so w is
//            NaN or 0 and the tap is skipped, as the definition's usable test does.
// A pass reads `in` and writes `out`, which never alias: passes ping-pong between d_out and
// d_work so that the last lands in d_out, and when the first would read what it writes
// (d_out == d_in, odd iters) the input is copied to d_work first.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dm_exp.h"
#include "dm_host.h"      // dm_fail, DM_HIP_TRY, dm_is_hole, dm_nan, dm_maps_plan, dm_tile_env

#define BIL_THREADS 256
#define BIL_TMAX 32                      // largest tile side
#define BIL_RMAX 15
#define BIL_WC 512                       // entries of the uint8 path's colour table
#define BIL_G_OUT 511                    // guide value of an unusable tap on that path

enum { GK_SELF = 0, GK_F64 = 1, GK_U8 = 2 };
// what a pass does with d_filled: nothing; 1 where the input is a hole and the output finite
// (the only pass); 1 where the input is a hole (first of several passes); the entry and the
// output is finite (last of several passes)
enum { FM_NONE = 0, FM_ONLY = 1, FM_FIRST = 2, FM_LAST = 3 };

// bytes of LDS of one workgroup: value plane, spatial table, then the guide plane / colour table
static size_t bil_lds(int gk, int T, int r)
{
    const size_t n = (size_t)(T + 2 * r) * (T + 2 * r), k = (size_t)(2 * r + 1) * (2 * r + 1);
    size_t b = (n + k) * sizeof(double);
    if (gk == GK_F64) b += n * sizeof(double);
    if (gk == GK_U8) b += BIL_WC * sizeof(double) + ((n * sizeof(uint16_t) + 15) & ~(size_t)15);
    return b;
}

// grid (tiles_x * tiles_y, M).  in / out [M][H][W]; guide [gmaps][H][W] (GK_F64: double,
// GK_U8: uint8_t, GK_SELF: unused).  T = 1 << ts.
template <int GK>
__global__ __launch_bounds__(BIL_THREADS) void k_bilat(const double *in, const void *guide, int gmaps, int H, int W,
                                                       int tiles_x, int ts, int r, double den_color,
                                                       double den_space, int fill, int fmode, double *out,
                                                       uint8_t *filled)
{
    extern __shared__ double bil_lds_[];
    const int T = 1 << ts, LW = T + 2 * r, n = LW * LW, D = 2 * r + 1, K = D * D;
    double *Xs = bil_lds_;
    double *Ws = Xs + n;
    double *Gs = GK == GK_F64 ? Ws + K : Xs;                    // GK_SELF: the value plane itself
    double *Wc = Ws + K;                                        // GK_U8 only
    uint16_t *Gu = (uint16_t *)(Wc + BIL_WC);                   // GK_U8 only

    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int y0 = tile_y << ts, x0 = tile_x << ts;
    const size_t cells = (size_t)H * W;
    const size_t mbase = (size_t)blockIdx.y * cells;
    const size_t gbase = gmaps == 1 ? 0 : mbase;
    const double *gd = (const double *)guide + gbase;
    const uint8_t *gu = (const uint8_t *)guide + gbase;
    in += mbase;

    for (int l = threadIdx.x; l < n; l += BIL_THREADS) {
        const int ly = l / LW, lx = l - ly * LW;
        const int y = y0 - r + ly, x = x0 - r + lx;
        const bool inside = y >= 0 && y < H && x >= 0 && x < W;
        const size_t c = inside ? (size_t)y * W + x : 0;
        const double v = inside ? in[c] : dm_nan();
        if (GK == GK_U8) {
            const bool usable = !dm_is_hole(v);                // (outside the map: NaN)
            Xs[l] = usable ? v : 0.0;
            Gu[l] = usable ? (uint16_t)gu[c] : (uint16_t)BIL_G_OUT;
        } else {
            Xs[l] = v;
            if (GK == GK_F64) {
                const double g = inside ? gd[c] : dm_nan();
                Gs[l] = (dm_is_hole(v) || dm_is_hole(g)) ? dm_nan() : g;
            }
        }
    }
    for (int k = threadIdx.x; k < K; k += BIL_THREADS) {
        const int dy = k / D - r, dx = k % D - r;
        Ws[k] = dm_exp(-(double)(dy * dy + dx * dx) / den_space);
    }
    if (GK == GK_U8)
        for (int k = threadIdx.x; k < BIL_WC; k += BIL_THREADS) {
            const double c = (double)k;
            Wc[k] = k < 256 ? dm_exp(-(c * c) / den_color) : 0.0;
        }
    __syncthreads();

    for (int l = threadIdx.x; l < T * T; l += BIL_THREADS) {
        const int ty = l >> ts, tx = l & (T - 1);
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const size_t c = (size_t)y * W + x;
        const double xc = in[c];
        const bool hole = dm_is_hole(xc);
        double res = xc;
        bool copy = hole && !fill;
        const int ctr = (ty + r) * LW + tx + r;
        if (GK == GK_U8) {
            if (!copy) {
                const int g0 = gu[c];
                double num = 0.0, den = 0.0;
                int k = 0;
                for (int dy = -r; dy <= r; ++dy) {
                    const int row = ctr + dy * LW - r;
                    for (int i = 0; i < D; ++i, ++k) {
                        const int d = g0 - (int)Gu[row + i];
                        const double w = Ws[k] * Wc[d < 0 ? -d : d];
                        num = num + w * Xs[row + i];
                        den = den + w;
                    }
                }
                if (den > 0.0) res = num / den;
            }
        } else {
            const double g0 = GK == GK_F64 ? gd[c] : xc;
            copy = copy || dm_is_hole(g0);
            if (!copy) {
                double num = 0.0, den = 0.0;
                int k = 0;
                for (int dy = -r; dy <= r; ++dy) {
                    const int row = ctr + dy * LW - r;
                    for (int i = 0; i < D; ++i, ++k) {
                        const double cd = g0 - Gs[row + i];
                        const double wc = dm_exp(-(cd * cd) / den_color);
                        const double w = Ws[k] * wc;
                        if (w > 0.0) {
                            num = num + w * Xs[row + i];
                            den = den + w;
                        }
                    }
                }
                if (den > 0.0) res = num / den;
            }
        }
        out[mbase + c] = res;      // (a copied cell: the double moves unchanged, payload and sign)
        if (fmode == FM_ONLY) filled[mbase + c] = hole && !dm_is_hole(res) ? 1 : 0;
        else if (fmode == FM_FIRST) filled[mbase + c] = hole ? 1 : 0;
        else if (fmode == FM_LAST) filled[mbase + c] = filled[mbase + c] && !dm_is_hole(res) ? 1 : 0;
    }
}

// ---- host side ------------------------------------------------------------------------------
// false for a shape the entry does not take (the limits of dm_fill_bytes)
static bool bil_plan(int32_t M, int32_t H, int32_t W, size_t *bytes)
{
    if (!dm_maps_plan(M, H, W, 64 * 65535)) return false;
    *bytes = ((size_t)M * H * W * sizeof(double) + 15) & ~(size_t)15;      // one plane for the ping-pong
    return true;
}

// log2 of the tile side (the result does not depend on it).  A tile of 32 has the smaller share
// of halo, but it pays only where eight workgroups of it fit the CU's 160 KB of LDS (32 waves:
// the uint8 path up to radius 3) and the grid has 4096 of them or more (16 per CU); elsewhere
// a tile of 16 keeps more waves on the CU (measured: DESIGN.md 4h).  DM_BILATERAL_TILE = 16 or
// 32 forces one, for measurements and tests.
static int bil_tile_shift(int gk, int32_t M, int32_t H, int32_t W, int r)
{
    if (const int ts = dm_tile_env("DM_BILATERAL_TILE")) return ts;
    const long long tiles = (long long)((H + 31) >> 5) * ((W + 31) >> 5) * M;
    return 8 * bil_lds(gk, 32, r) <= 160 * 1024 && tiles >= 4096 ? 5 : 4;
}

template <int GK>
static hipError_t bil_launch(const double *in, const void *guide, int gmaps, int M, int H, int W, int ts, int r,
                             double den_color, double den_space, int fill, int fmode, double *out,
                             uint8_t *filled, hipStream_t st)
{
    const int T = 1 << ts;
    const int tiles_x = (W + T - 1) >> ts, tiles_y = (H + T - 1) >> ts;      // tiles_x tiles_y < 2^24
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, M);
    k_bilat<GK><<<grid, BIL_THREADS, bil_lds(GK, T, r), st>>>(in, guide, gmaps, H, W, tiles_x, ts, r, den_color,
                                                              den_space, fill, fmode, out, filled);
    return hipGetLastError();
}

extern "C" {

size_t dm_bilateral_bytes(int32_t M, int32_t H, int32_t W)
{
    size_t b;
    return bil_plan(M, H, W, &b) ? b : 0;
}

int dm_bilateral_filter(const double *d_in, const void *d_guide, int32_t guide_maps, int32_t M, int32_t H,
                        int32_t W, int32_t radius, double den_color, double den_space, int32_t iters,
                        int32_t flags, double *d_out, uint8_t *d_filled, void *d_work, void *stream)
{
    if (!d_in || !d_out || !d_work) return dm_fail(DM_ERR_ARG, "null input / output / workspace pointer");
    if (M < 1 || H < 1 || W < 1) return dm_fail(DM_ERR_ARG, "bad bilateral shape M=%d H=%d W=%d", M, H, W);
    if (radius < 1 || radius > BIL_RMAX) return dm_fail(DM_ERR_ARG, "radius must be in [1, %d] (got %d)", BIL_RMAX, radius);
    if (iters < 1 || iters > 64) return dm_fail(DM_ERR_ARG, "iters must be in [1, 64] (got %d)", iters);
    if (!(den_color > 0.0)) return dm_fail(DM_ERR_ARG, "den_color must be > 0 (got %g)", den_color);
    if (!(den_space > 0.0)) return dm_fail(DM_ERR_ARG, "den_space must be > 0 (got %g)", den_space);
    if (flags & ~(DM_BILAT_FILL | DM_BILAT_GUIDE_U8)) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    if (d_guide) {
        if (guide_maps != 1 && guide_maps != M)
            return dm_fail(DM_ERR_ARG, "guide_maps must be 1 or M=%d (got %d)", M, guide_maps);
    } else if (flags & (DM_BILAT_FILL | DM_BILAT_GUIDE_U8)) {
        return dm_fail(DM_ERR_ARG, "flags 0x%x need a guide", flags);
    }
    size_t bytes;
    if (!bil_plan(M, H, W, &bytes))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "bilateral filter of %d maps of %d x %d cells (at most 65535 maps of 2^31 - 1 cells)", M, H, W);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_set = false; // idempotent attributes, benign race
    if (!attr_set) {
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_bilat<GK_SELF>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bil_lds(GK_SELF, BIL_TMAX, BIL_RMAX)));
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_bilat<GK_F64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bil_lds(GK_F64, BIL_TMAX, BIL_RMAX)));
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_bilat<GK_U8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bil_lds(GK_U8, BIL_TMAX, BIL_RMAX)));
        attr_set = true;
    }
    const int gk = !d_guide ? GK_SELF : (flags & DM_BILAT_GUIDE_U8) ? GK_U8 : GK_F64;
    const int ts = bil_tile_shift(gk, M, H, W, radius);
    const int fill = (flags & DM_BILAT_FILL) ? 1 : 0;
    double *work = (double *)d_work;
    // pass p writes d_out when an even number of passes follow it, else d_work
    const double *src = d_in;
    if (d_in == d_out && (iters & 1)) {      // the first pass would read what it writes
        DM_HIP_TRY(hipMemcpyAsync(work, d_in, (size_t)M * H * W * sizeof(double), hipMemcpyDeviceToDevice, st));
        src = work;
    }
    for (int p = 0; p < iters; ++p) {
        double *dst = ((iters - 1 - p) & 1) ? work : d_out;
        const int fmode = !d_filled ? FM_NONE : iters == 1 ? FM_ONLY : p == 0 ? FM_FIRST : p == iters - 1 ? FM_LAST : FM_NONE;
        hipError_t e;
        if (gk == GK_U8)
            e = bil_launch<GK_U8>(src, d_guide, guide_maps, M, H, W, ts, radius, den_color, den_space, fill, fmode, dst, d_filled, st);
        else if (gk == GK_F64)
            e = bil_launch<GK_F64>(src, d_guide, guide_maps, M, H, W, ts, radius, den_color, den_space, fill, fmode, dst, d_filled, st);
        else
            e = bil_launch<GK_SELF>(src, nullptr, 1, M, H, W, ts, radius, den_color, den_space, fill, fmode, dst, d_filled, st);
        DM_HIP_TRY(e);
        src = dst;
    }
    return DM_OK;
}

} // extern "C"
