// dm_fill.hip -- gfx950 kernels + C ABI of the hole fill: cascadic push-pull with masked
// Jacobi relaxation (dm_fill_holes, include/dmstereo.h).
//
// A hole is a non-finite cell.  Level 0 is the map with holes as (v = 0, n = 0) and finite
// cells as (v = x, n = 1); level k + 1 has sides ceil(h / 2), ceil(w / 2):
//
//   pull   s = ((n00 v00 + n01 v01) + n10 v10) + n11 v11;  m = ((n00 + n01) + n10) + n11
//          v' = m > 0 ? s / m : 0;  n' = m            (children outside the level: v = n = 0)
//   push   a cell with n == 0 takes (((9 a + 3 b) + 3 c) + d) / 16 of the finished level k + 1,
//          a = p[I][J], b = p[I2][J], c = p[I][J2], d = p[I2][J2], I = i >> 1, I2 = I -+ 1 by
//          the parity of i, clamped (J likewise)
//   relax  `iters` Jacobi steps on the cells with n == 0: (((U + D) + L) + R) / 4, neighbours
//          index-clamped, every read from the previous iterate
//
// from the 1 x 1 top down, push then relax at EVERY level.  float64, no contraction
// (-ffp-contract=off), the parenthesised order above: the result equals the numpy restatement
// in tests/test_fill_host.py bit for bit.  A map that is all holes is copied unchanged.
//
// Launch count is the cost (a 1024^2 map has 11 levels; one launch per pull, push and Jacobi
// step would be ~190 dependent launches), so:
//   k_fill_pull  one workgroup reduces a 64 x 64 block of its source level by up to 6 levels
//                (32^2 ... 1^2 in LDS), writing each level's v, n and hole mask;
//   k_fill_top   one workgroup per map holds every level from the first of <= FILL_TOPC cells
//                up to 1 x 1 in LDS and runs their pulls, pushes and relaxations there;
//   k_fill_tile  a larger level in tiles of FILL_T^2 cells plus a halo of s <= FILL_K cells:
//                push from the parent level (first launch of the level), s Jacobi steps in LDS,
//                write the tile.  Step t only has to be right s - t cells outside the tile, and
//                a Jacobi step is local, so this equals s whole-map steps bit for bit.
// Only hole cells are relaxed: both LDS iterates start as the pushed level, so a finite cell
// reads the same from either.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dm_host.h"      // dm_fail, DM_HIP_TRY, dm_is_hole, dm_maps_plan

#define FILL_T 64                       // tile side of k_fill_tile
#define FILL_K 16                       // its largest halo = Jacobi steps per launch
#define FILL_R (FILL_T + 2 * FILL_K)    // side of the LDS region
#define FILL_TOPC 4096                  // k_fill_top takes the first level of at most this many cells
#define FILL_TOPCAP 8256                // cells of that level and all above it: <= 2 * 4096 + 13 (a 1 x 4096 level)
#define FILL_PULL 6                     // levels one k_fill_pull launch produces (64 = 2^6)
#define FILL_MAXLEV 33
#define FILL_THREADS 1024

static constexpr size_t FILL_TILE_LDS = (size_t)FILL_R * FILL_R * (2 * sizeof(double) + 1);
static constexpr size_t FILL_TOP_LDS = (size_t)FILL_TOPCAP * (sizeof(double) + sizeof(uint32_t)) +
                                       (size_t)FILL_TOPC * sizeof(double);

__device__ __forceinline__ double fill_pull_cell(double v00, double v01, double v10, double v11, uint32_t n00,
                                                 uint32_t n01, uint32_t n10, uint32_t n11, uint32_t *m)
{
    const double s = (((double)n00 * v00 + (double)n01 * v01) + (double)n10 * v10) + (double)n11 * v11;
    *m = n00 + n01 + n10 + n11;      // exact: at most H W <= 2^31 - 1 finite cells
    return *m > 0 ? s / (double)*m : 0.0;
}

// the 9/3/3/1 interpolation of level k + 1 (p, ph x pw) at cell (i, j) of level k
__device__ __forceinline__ double fill_push_cell(const double *p, int ph, int pw, int i, int j)
{
    const int I = i >> 1, J = j >> 1;
    const int I2 = min(max(I + ((i & 1) ? 1 : -1), 0), ph - 1);
    const int J2 = min(max(J + ((j & 1) ? 1 : -1), 0), pw - 1);
    const double a = p[(size_t)I * pw + J], b = p[(size_t)I2 * pw + J];
    const double c = p[(size_t)I * pw + J2], d = p[(size_t)I2 * pw + J2];
    return (((9.0 * a + 3.0 * b) + 3.0 * c) + d) * 0.0625;
}

// one Jacobi step of cell (i, j) of an h x w array of row pitch w, neighbours index-clamped
__device__ __forceinline__ double fill_relax_cell(const double *v, int h, int w, int i, int j)
{
    const double U = v[max(i - 1, 0) * w + j], D = v[min(i + 1, h - 1) * w + j];
    const double Lf = v[i * w + max(j - 1, 0)], R = v[i * w + min(j + 1, w - 1)];
    return (((U + D) + Lf) + R) * 0.25;
}

struct FillPullOut {
    double *v[FILL_PULL];
    uint32_t *n[FILL_PULL];
    uint8_t *hole[FILL_PULL];
    int h[FILL_PULL], w[FILL_PULL];
};

// Levels src + 1 .. src + nl from level src (h x w).  srcn == NULL: the source is the input
// map itself (level 0): holes are found here and written to hole0.  grid (ceil(w / 64),
// ceil(h / 64), M), 256 threads; every array is [M][cells of its level].
__global__ __launch_bounds__(256) void k_fill_pull(const double *src, const uint32_t *srcn, int h, int w, int nl,
                                                   uint8_t *hole0, FillPullOut o)
{
    __shared__ double sv[2][32 * 32];
    __shared__ uint32_t sn[2][32 * 32];
    const int m = blockIdx.z;
    const size_t c0 = (size_t)h * w;
    src += m * c0;
    if (srcn) srcn += m * c0;
    else hole0 += m * c0;
    // stage 1: 32 x 32 cells of level src + 1 from global memory
    {
        const int h1 = o.h[0], w1 = o.w[0];
        double *ov = o.v[0] + (size_t)m * h1 * w1;
        uint32_t *on = o.n[0] + (size_t)m * h1 * w1;
        uint8_t *oh = o.hole[0] + (size_t)m * h1 * w1;
        for (int l = threadIdx.x; l < 32 * 32; l += 256) {
            const int I = blockIdx.y * 32 + (l >> 5), J = blockIdx.x * 32 + (l & 31);
            double cv[4];
            uint32_t cn[4];
            for (int q = 0; q < 4; ++q) {
                const int i = 2 * I + (q >> 1), j = 2 * J + (q & 1);
                cv[q] = 0.0;
                cn[q] = 0;
                if (i < h && j < w) {
                    const size_t g = (size_t)i * w + j;
                    const double x = src[g];
                    if (srcn) {
                        cv[q] = x;
                        cn[q] = srcn[g];
                    } else {
                        const bool hole = dm_is_hole(x);
                        hole0[g] = hole ? 1 : 0;
                        cv[q] = hole ? 0.0 : x;
                        cn[q] = hole ? 0 : 1;
                    }
                }
            }
            uint32_t mm;
            const double v = fill_pull_cell(cv[0], cv[1], cv[2], cv[3], cn[0], cn[1], cn[2], cn[3], &mm);
            sv[0][l] = v;      // (a cell outside the level holds v = 0, n = 0)
            sn[0][l] = mm;
            if (I < h1 && J < w1) {
                const size_t g = (size_t)I * w1 + J;
                ov[g] = v;
                on[g] = mm;
                oh[g] = mm == 0 ? 1 : 0;
            }
        }
    }
    // stages 2 .. nl: (32 >> (s - 1))^2 cells each, from the previous stage in LDS
    for (int s = 1; s < nl; ++s) {
        __syncthreads();
        const int side = 32 >> s, ps = side * 2;
        const double *pv = sv[(s - 1) & 1];
        const uint32_t *pn = sn[(s - 1) & 1];
        const int hs = o.h[s], ws = o.w[s];
        for (int l = threadIdx.x; l < side * side; l += 256) {
            const int li = l / side, lj = l % side;
            const int a = (2 * li) * ps + 2 * lj;
            uint32_t mm;
            const double v = fill_pull_cell(pv[a], pv[a + 1], pv[a + ps], pv[a + ps + 1], pn[a], pn[a + 1],
                                            pn[a + ps], pn[a + ps + 1], &mm);
            sv[s & 1][l] = v;
            sn[s & 1][l] = mm;
            const int I = blockIdx.y * side + li, J = blockIdx.x * side + lj;
            if (I < hs && J < ws) {
                const size_t g = (size_t)m * hs * ws + (size_t)I * ws + J;
                o.v[s][g] = v;
                o.n[s][g] = mm;
                o.hole[s][g] = mm == 0 ? 1 : 0;
            }
        }
    }
}

// The pyramid top of one map per workgroup: the h x w level in src (srcn == NULL: the input
// map itself, holes found here and written to `holes` if given; else values and counts of a
// pulled level) and every level above it live in LDS; pull up to 1 x 1, then push + relax back
// down and write the finished h x w level to dst (which may be src).  total[m] receives the
// map's count of finite cells.  An all-hole input map is copied bit for bit.
__global__ __launch_bounds__(FILL_THREADS) void k_fill_top(const double *src, const uint32_t *srcn, int h, int w,
                                                           int iters, double *dst, uint8_t *holes, uint32_t *total)
{
    extern __shared__ double fill_lds[];
    double *V = fill_lds;                         // [FILL_TOPCAP] values of every level
    double *S = V + FILL_TOPCAP;                  // [FILL_TOPC] the second Jacobi iterate
    uint32_t *N = (uint32_t *)(S + FILL_TOPC);    // [FILL_TOPCAP] counts
    __shared__ int lh[FILL_MAXLEV], lw[FILL_MAXLEV], off[FILL_MAXLEV], nlev;
    const int m = blockIdx.x, tid = threadIdx.x;
    const int c0 = h * w;
    src += (size_t)m * c0;
    dst += (size_t)m * c0;
    if (srcn) srcn += (size_t)m * c0;
    if (holes) holes += (size_t)m * c0;
    if (tid == 0) {
        int k = 0, o = 0;
        lh[0] = h;
        lw[0] = w;
        off[0] = 0;
        while (lh[k] > 1 || lw[k] > 1) {
            o += lh[k] * lw[k];
            lh[k + 1] = (lh[k] + 1) >> 1;
            lw[k + 1] = (lw[k] + 1) >> 1;
            off[++k] = o;
        }
        nlev = k + 1;
    }
    for (int l = tid; l < c0; l += FILL_THREADS) {
        const double x = src[l];
        if (srcn) {
            V[l] = x;
            N[l] = srcn[l];
        } else {
            const bool hole = dm_is_hole(x);
            V[l] = hole ? 0.0 : x;
            N[l] = hole ? 0 : 1;
            if (holes) holes[l] = hole ? 1 : 0;
        }
    }
    __syncthreads();
    const int nl = nlev;
    for (int k = 0; k + 1 < nl; ++k) {
        const int hk = lh[k], wk = lw[k], h1 = lh[k + 1], w1 = lw[k + 1];
        const double *pv = V + off[k];
        const uint32_t *pn = N + off[k];
        for (int l = tid; l < h1 * w1; l += FILL_THREADS) {
            const int I = l / w1, J = l % w1;
            double cv[4];
            uint32_t cn[4];
            for (int q = 0; q < 4; ++q) {
                const int i = 2 * I + (q >> 1), j = 2 * J + (q & 1);
                const bool in = i < hk && j < wk;
                cv[q] = in ? pv[i * wk + j] : 0.0;
                cn[q] = in ? pn[i * wk + j] : 0;
            }
            uint32_t mm;
            V[off[k + 1] + l] = fill_pull_cell(cv[0], cv[1], cv[2], cv[3], cn[0], cn[1], cn[2], cn[3], &mm);
            N[off[k + 1] + l] = mm;
        }
        __syncthreads();
    }
    const uint32_t tot = N[off[nl - 1]];
    if (tid == 0) total[m] = tot;
    if (tot == 0) {      // nothing to fill from (uniform over the workgroup)
        if (!srcn)
            for (int l = tid; l < c0; l += FILL_THREADS) dst[l] = src[l];
        return;
    }
    for (int k = nl - 2; k >= 0; --k) {
        const int hk = lh[k], wk = lw[k], ck = hk * wk;
        double *v = V + off[k];
        const uint32_t *n = N + off[k];
        const double *p = V + off[k + 1];
        for (int l = tid; l < ck; l += FILL_THREADS) {
            double x = v[l];
            if (n[l] == 0) {
                x = fill_push_cell(p, lh[k + 1], lw[k + 1], l / wk, l % wk);
                v[l] = x;
            }
            S[l] = x;
        }
        __syncthreads();
        double *cur = v, *oth = S;
        for (int t = 0; t < iters; ++t) {
            for (int l = tid; l < ck; l += FILL_THREADS)
                if (n[l] == 0) oth[l] = fill_relax_cell(cur, hk, wk, l / wk, l % wk);
            __syncthreads();
            double *x = cur;
            cur = oth;
            oth = x;
        }
        if (cur != v) {
            for (int l = tid; l < ck; l += FILL_THREADS)
                if (n[l] == 0) v[l] = S[l];
            __syncthreads();
        }
    }
    for (int l = tid; l < c0; l += FILL_THREADS) dst[l] = V[l];
}

// One tile of an H x W level: the tile plus a halo of `steps` cells (clipped to the level) goes
// to LDS, `steps` Jacobi steps run there on the hole cells, the tile is written to dst.
// first: src is the level as pulled (level 0: the input map) and hole cells take the push from
// parent (ph x pw) instead of src, so an in-place level 0 never reads a cell another workgroup
// writes.  Otherwise src is the previous launch's iterate; src != dst then.  total (level 0
// only): a map without a finite cell is copied through unchanged.  grid (ceil(W / FILL_T),
// ceil(H / FILL_T), M).
__global__ __launch_bounds__(FILL_THREADS) void k_fill_tile(const double *src, int first, const uint8_t *hole,
                                                            const double *parent, int ph, int pw, double *dst,
                                                            int H, int W, int steps, const uint32_t *total)
{
    extern __shared__ double fill_lds[];
    const int m = blockIdx.z;
    const size_t cells = (size_t)H * W;
    src += m * cells;
    dst += m * cells;
    hole += m * cells;
    const int y0 = blockIdx.y * FILL_T, x0 = blockIdx.x * FILL_T;
    const int y1 = min(y0 + FILL_T, H), x1 = min(x0 + FILL_T, W);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (total && total[m] == 0) {
        for (int y = y0 + ty; y < y1; y += 32)
            for (int x = x0 + tx; x < x1; x += 32) dst[(size_t)y * W + x] = src[(size_t)y * W + x];
        return;
    }
    if (first) parent += (size_t)m * ph * pw;
    const int ry0 = max(y0 - steps, 0), ry1 = min(y1 + steps, H);
    const int rx0 = max(x0 - steps, 0), rx1 = min(x1 + steps, W);
    const int rh = ry1 - ry0, rw = rx1 - rx0;      // <= FILL_R: steps <= FILL_K
    double *A = fill_lds, *B = A + FILL_R * FILL_R;
    uint8_t *mask = (uint8_t *)(B + FILL_R * FILL_R);
    for (int ly = ty; ly < rh; ly += 32)
        for (int lx = tx; lx < rw; lx += 32) {
            const int gy = ry0 + ly, gx = rx0 + lx;
            const size_t g = (size_t)gy * W + gx;
            const uint8_t hf = hole[g];
            const double v = (first && hf) ? fill_push_cell(parent, ph, pw, gy, gx) : src[g];
            const int l = ly * rw + lx;
            A[l] = v;
            B[l] = v;
            mask[l] = hf;
        }
    __syncthreads();
    double *cur = A, *oth = B;
    for (int t = 1; t <= steps; ++t) {
        // right after step t: every cell t or more cells inside the region's edges that are not
        // edges of the level (the clamp at a level edge is the definition's own)
        const int cy0 = ry0 == 0 ? 0 : t, cy1 = ry1 == H ? rh : rh - t;
        const int cx0 = rx0 == 0 ? 0 : t, cx1 = rx1 == W ? rw : rw - t;
        for (int ly = cy0 + ty; ly < cy1; ly += 32)
            for (int lx = cx0 + tx; lx < cx1; lx += 32)
                if (mask[ly * rw + lx]) oth[ly * rw + lx] = fill_relax_cell(cur, rh, rw, ly, lx);
        __syncthreads();
        double *x = cur;
        cur = oth;
        oth = x;
    }
    for (int y = y0 + ty; y < y1; y += 32)
        for (int x = x0 + tx; x < x1; x += 32) dst[(size_t)y * W + x] = cur[(y - ry0) * rw + (x - rx0)];
}

// ---- host side ------------------------------------------------------------------------------
struct FillPlan {
    int nlev, ktop;                      // levels 0 .. nlev - 1; k_fill_top takes ktop and above
    int h[FILL_MAXLEV], w[FILL_MAXLEV];
    size_t total, t0, hole0;             // byte offsets into the workspace
    size_t v[FILL_MAXLEV], b[FILL_MAXLEV], n[FILL_MAXLEV], hole[FILL_MAXLEV];   // levels 1 .. ktop
    size_t bytes;
};

static size_t fill_take(size_t *off, size_t bytes)
{
    const size_t at = *off;
    *off += (bytes + 15) & ~(size_t)15;
    return at;
}

// false for a shape the entry does not take
static bool fill_plan(int32_t M, int32_t H, int32_t W, FillPlan *p)
{
    if (!dm_maps_plan(M, H, W, 64 * 65535)) return false;      // grid y / z
    int k = 0;
    p->h[0] = H;
    p->w[0] = W;
    while (p->h[k] > 1 || p->w[k] > 1) {
        p->h[k + 1] = (p->h[k] + 1) >> 1;
        p->w[k + 1] = (p->w[k] + 1) >> 1;
        ++k;
    }
    p->nlev = k + 1;
    p->ktop = 0;
    while ((long long)p->h[p->ktop] * p->w[p->ktop] > FILL_TOPC) ++p->ktop;
    size_t off = 0;
    const size_t c0 = (size_t)H * W;
    p->total = fill_take(&off, (size_t)M * sizeof(uint32_t));
    p->t0 = fill_take(&off, (size_t)M * c0 * sizeof(double));
    p->hole0 = fill_take(&off, (size_t)M * c0);
    for (k = 1; k <= p->ktop; ++k) {
        const size_t c = (size_t)M * p->h[k] * p->w[k];
        p->v[k] = fill_take(&off, c * sizeof(double));
        p->b[k] = fill_take(&off, c * sizeof(double));
        p->n[k] = fill_take(&off, c * sizeof(uint32_t));
        p->hole[k] = fill_take(&off, c);
    }
    p->bytes = off;
    return true;
}

// Jacobi steps per k_fill_tile launch: FILL_K, or DM_FILL_STEPS (1 .. FILL_K) for measurements
// (1 is the plain one-step-per-launch relaxation; the result does not depend on it)
static int fill_steps_per_launch()
{
    const char *e = getenv("DM_FILL_STEPS");
    if (!e || !*e) return FILL_K;
    const int v = atoi(e);
    return v < 1 ? 1 : v > FILL_K ? FILL_K : v;
}

extern "C" {

size_t dm_fill_bytes(int32_t M, int32_t H, int32_t W)
{
    FillPlan p;
    return fill_plan(M, H, W, &p) ? p.bytes : 0;
}

int dm_fill_holes(const double *d_in, int32_t M, int32_t H, int32_t W, int32_t iters, double *d_out,
                  uint8_t *d_holes, void *d_work, void *stream)
{
    if (!d_in || !d_out || !d_work) return dm_fail(DM_ERR_ARG, "null input / output / workspace pointer");
    if (M < 1 || H < 1 || W < 1) return dm_fail(DM_ERR_ARG, "bad fill shape M=%d H=%d W=%d", M, H, W);
    if (iters < 0 || iters > 4096) return dm_fail(DM_ERR_ARG, "iterations must be in [0, 4096] (got %d)", iters);
    FillPlan p;
    if (!fill_plan(M, H, W, &p))
        return dm_fail(DM_ERR_UNSUPPORTED, "fill of %d maps of %d x %d cells (at most 65535 maps of 2^31 - 1 cells)",
                     M, H, W);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_set = false; // idempotent attributes, benign race
    if (!attr_set) {
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_fill_top, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)FILL_TOP_LDS));
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_fill_tile, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)FILL_TILE_LDS));
        attr_set = true;
    }
    char *ws = (char *)d_work;
    uint32_t *total = (uint32_t *)(ws + p.total);
    if (p.ktop == 0) {      // the whole pyramid in one launch
        k_fill_top<<<M, FILL_THREADS, FILL_TOP_LDS, st>>>(d_in, nullptr, H, W, iters, d_out, d_holes, total);
        DM_HIP_TRY(hipGetLastError());
        return DM_OK;
    }
    uint8_t *hole0 = d_holes ? d_holes : (uint8_t *)(ws + p.hole0);
    for (int s = 0; s < p.ktop;) {
        const int nl = p.ktop - s < FILL_PULL ? p.ktop - s : FILL_PULL;
        FillPullOut o = {};
        for (int q = 0; q < nl; ++q) {
            const int k = s + 1 + q;
            o.v[q] = (double *)(ws + p.v[k]);
            o.n[q] = (uint32_t *)(ws + p.n[k]);
            o.hole[q] = (uint8_t *)(ws + p.hole[k]);
            o.h[q] = p.h[k];
            o.w[q] = p.w[k];
        }
        const dim3 grid((p.w[s] + 63) / 64, (p.h[s] + 63) / 64, M);
        k_fill_pull<<<grid, 256, 0, st>>>(s ? (const double *)(ws + p.v[s]) : d_in,
                                          s ? (const uint32_t *)(ws + p.n[s]) : nullptr, p.h[s], p.w[s], nl, hole0, o);
        DM_HIP_TRY(hipGetLastError());
        s += nl;
    }
    double *parent = (double *)(ws + p.v[p.ktop]);
    k_fill_top<<<M, FILL_THREADS, FILL_TOP_LDS, st>>>(parent, (const uint32_t *)(ws + p.n[p.ktop]), p.h[p.ktop],
                                                      p.w[p.ktop], iters, parent, nullptr, total);
    DM_HIP_TRY(hipGetLastError());
    const int per = fill_steps_per_launch();
    const int launches = iters ? (iters + per - 1) / per : 1;
    for (int k = p.ktop - 1; k >= 0; --k) {
        // the iterate alternates between two buffers, never the one it is read from; level 0
        // ends in d_out
        const double *src = k ? (const double *)(ws + p.v[k]) : d_in;
        double *buf[2] = {k ? (double *)(ws + p.b[k]) : d_out, k ? (double *)(ws + p.v[k]) : (double *)(ws + p.t0)};
        const uint8_t *hole = k ? (const uint8_t *)(ws + p.hole[k]) : hole0;
        const dim3 grid((p.w[k] + FILL_T - 1) / FILL_T, (p.h[k] + FILL_T - 1) / FILL_T, M);
        int done = 0;
        for (int j = 0; j < launches; ++j) {
            const int steps = iters - done < per ? iters - done : per;
            double *dst = buf[(k ? j : launches - 1 - j) & 1];
            k_fill_tile<<<grid, FILL_THREADS, FILL_TILE_LDS, st>>>(src, j == 0, hole, parent, p.h[k + 1], p.w[k + 1],
                                                                   dst, p.h[k], p.w[k], steps, k ? nullptr : total);
            DM_HIP_TRY(hipGetLastError());
            done += steps;
            src = dst;
        }
        parent = (double *)src;
    }
    return DM_OK;
}

} // extern "C"
