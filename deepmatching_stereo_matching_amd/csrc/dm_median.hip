// dm_median.hip -- gfx950 kernel + C ABI of the NaN-aware weighted median filter
// (dm_median_filter, include/dmstereo.h).
//
// One pass, input X, optional weights Wt.  key(x) is the order-preserving 64-bit integer of a
// double (sign set: all bits flipped, else the sign bit set).  A tap is usable when it lies
// inside the map, X is finite there (range test on the double) and, with weights, w > 0 and
// w < +inf.  A hole without DM_MEDIAN_FILL, and a cell with fewer than min_count usable taps,
// is copied bit for bit.  Otherwise, over the usable taps in window order (dy = -r .. r outer,
// dx = -r .. r inner):
//   unweighted  the tap value of rank (n - 1) / 2 by key
//   weighted    T = the sequential float64 sum of the weights, S(v) the same sum over the taps
//               with key <= key(v); the smallest tap value v with S(v) >= 0.5 T
// tests/test_median_host.py restates this in plain loops (median_restate); the kernel equals
// it bit for bit, whatever the tile side.
//
// k_median<WT, R>: one launch per pass, one workgroup of 256 threads per tile of T x T cells
// (T = 16 or 32: med_tile_shift), grid (tiles, M).  The tile with its halo of r cells is staged
// into LDS as keys; an unusable tap (out of the map, a hole, an unusable weight) holds the
// sentinel key of all ones -- the key of a NaN, so no usable tap has it -- and the weight +0.
// A thread then selects the value of each of its T T / 256 cells on its own: no atomics, no
// cross-lane step, so the result depends neither on T nor on the schedule.
//
// The selection (med_select) is a bisection on the key, most significant bit first, that snaps
// to the window's own keys.  A first sweep of the window gives n, lo and hi, the smallest and
// the largest usable key (and T); the answer is a tap's key in [lo, hi].  While lo != hi, the
// candidate is their common leading bits followed by a one and zeros (lo < candidate <= hi),
// and one sweep of the window gives
//   unweighted  c = the number of taps with key < candidate; the answer is >= candidate
//               when c <= rank
//   weighted    s = the sum, in window order, of the weights of the taps with key < candidate;
//               the answer is >= candidate when s < 0.5 T
// together with the largest key below the candidate and the smallest key not below it; lo
// becomes the latter when the answer is >= candidate, else hi becomes the former.  Either way
// the highest bit in which lo and hi differ moves down, so there are at most 64 sweeps; as the
// bounds are taps, a window of n distinct values spread over its range takes about log2 n, and
// a constant window none.
// The sentinel is never below a candidate, and a tap that is not below it adds +0 to s, which
// changes no bit of a sum that starts at +0 and only has terms >= +0.  s is therefore the
// definition's S at the largest tap below the candidate (the sum over a down-set in window
// order); S is monotone, so "s < 0.5 T" holds exactly for the candidates up to the key of the
// definition's output, and with weights of 1.0 it is c <= (n - 1) / 2.  (0.5 T underflows to 0
// when T is the smallest denormal; no candidate then passes and hi comes down to the smallest
// key, the definition's answer.)
//   R = 1, 2, 3 (unweighted) and R = 1, 2 (weighted): the window is first copied from LDS into
//   registers, 9 / 25 / 49 keys, and the sweeps run on those.  R = 0: any radius, the sweeps
//   read LDS.
// A pass reads `in` and writes `out`, which never alias.  Out of place the passes ping-pong
// between d_out and the first plane of d_work so that the last lands in d_out.  In place
// (d_out == d_in) a single pass reads a copy of the input in d_work; several passes run
// through the two planes of d_work and only the last writes d_out, so that it still finds the
// input's bits there for d_changed: a thread reads its own cell of d_in before it writes it.
#include <hip/hip_runtime.h>

#include "dm_host.h"      // dm_fail, DM_HIP_TRY, dm_is_hole, dm_maps_plan, dm_tile_env

#define MED_THREADS 256
#define MED_RMAX 7
#define MED_SENT 0xffffffffffffffffULL      // key of an unusable tap
#define MED_SIGN 0x8000000000000000ULL

__device__ __forceinline__ uint64_t med_key(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b & MED_SIGN) ? ~b : (b | MED_SIGN);
}

__device__ __forceinline__ double med_value(uint64_t k)
{
    return __longlong_as_double((long long)((k & MED_SIGN) ? (k ^ MED_SIGN) : ~k));
}

// the window of one cell in LDS: ctr its centre, LW the row pitch
struct MedWinLds {
    const uint64_t *Ks;
    const double *Ws;
    int ctr, LW, r;
    template <int WT, class F>
    __device__ __forceinline__ void each(F f) const
    {
        const int D = 2 * r + 1;
        for (int dy = -r; dy <= r; ++dy) {
            const int row = ctr + dy * LW - r;
            for (int i = 0; i < D; ++i) f(Ks[row + i], WT ? Ws[row + i] : 0.0);
        }
    }
};

// the same window copied into registers (R known at compile time, every loop unrolled)
template <int WT, int R>
struct MedWinReg {
    static constexpr int D = 2 * R + 1, K = D * D;
    uint64_t k[K];
    double w[WT ? K : 1];
    __device__ __forceinline__ MedWinReg(const uint64_t *Ks, const double *Ws, int ctr, int LW)
    {
#pragma unroll
        for (int dy = 0; dy < D; ++dy)
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int l = ctr + (dy - R) * LW - R + i;
                k[dy * D + i] = Ks[l];
                if (WT) w[dy * D + i] = Ws[l];
            }
    }
    template <int WT_, class F>
    __device__ __forceinline__ void each(F f) const
    {
#pragma unroll
        for (int t = 0; t < K; ++t) f(k[t], WT ? w[WT ? t : 0] : 0.0);
    }
};

// false: fewer than min_count usable taps.  Else *out = the key of the (weighted) lower median.
template <int WT, class Win>
__device__ __forceinline__ bool med_select(const Win &win, int min_count, uint64_t *out)
{
    uint64_t lo = MED_SENT, hi = 0;
    int n = 0;
    double tot = 0.0;
    win.template each<WT>([&](uint64_t k, double w) {
        const bool u = k != MED_SENT;
        n += u ? 1 : 0;
        lo = k < lo ? k : lo;
        hi = (u && k > hi) ? k : hi;
        if (WT) tot = tot + w;
    });
    if (n < min_count) return false;      // (min_count >= 1: a window without a usable tap ends here)
    const double half = 0.5 * tot;
    const int rank = (n - 1) >> 1;
    while (lo != hi) {      // lo and hi are keys of usable taps and the answer lies in [lo, hi]
        const int b = 63 - __clzll((long long)(lo ^ hi));
        const uint64_t cand = (hi >> b) << b;      // the common prefix, then bit b: lo < cand <= hi
        uint64_t below = 0, above = MED_SENT;      // the largest key < cand, the smallest key >= cand
        bool up;                                   // the answer is >= cand
        if (WT) {
            double s = 0.0;
            win.template each<WT>([&](uint64_t k, double w) {
                const bool lt = k < cand;
                s = s + (lt ? w : 0.0);
                below = (lt && k > below) ? k : below;
                above = (!lt && k < above) ? k : above;
            });
            up = s < half;
        } else {
            int c = 0;
            win.template each<WT>([&](uint64_t k, double) {
                const bool lt = k < cand;
                c += lt ? 1 : 0;
                below = (lt && k > below) ? k : below;
                above = (!lt && k < above) ? k : above;
            });
            up = c <= rank;
        }
        if (up) lo = above;
        else hi = below;
    }
    *out = lo;
    return true;
}

// bytes of LDS of one workgroup: the key plane, then the weight plane
static size_t med_lds(int wt, int T, int r)
{
    const size_t n = (size_t)(T + 2 * r) * (T + 2 * r);
    return n * sizeof(uint64_t) * (wt ? 2 : 1);
}

// grid (tiles_x * tiles_y, M).  in / out [M][H][W]; weight [wmaps][H][W] (WT only).  T = 1 << ts.
// R: the radius when it is 1, 2 or 3 and the register path serves it, else 0 and the radius is rr.
// orig / changed: not NULL in the last pass of a call that asks for d_changed; orig is d_in.
template <int WT, int R>
__global__ __launch_bounds__(MED_THREADS) void k_median(const double *in, const double *weight, int wmaps, int H,
                                                        int W, int tiles_x, int ts, int rr, int min_count,
                                                        int fill, double *out, const double *orig,
                                                        uint8_t *changed)
{
    extern __shared__ uint64_t med_lds_[];
    const int r = R ? R : rr;
    const int T = 1 << ts, LW = T + 2 * r, n = LW * LW;
    uint64_t *Ks = med_lds_;
    double *Ws = (double *)(Ks + n);                            // WT only

    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int y0 = tile_y << ts, x0 = tile_x << ts;
    const size_t cells = (size_t)H * W;
    const size_t mbase = (size_t)blockIdx.y * cells;
    if (WT) weight += wmaps == 1 ? 0 : mbase;
    in += mbase;

    for (int l = threadIdx.x; l < n; l += MED_THREADS) {
        const int ly = l / LW, lx = l - ly * LW;
        const int y = y0 - r + ly, x = x0 - r + lx;
        const bool inside = y >= 0 && y < H && x >= 0 && x < W;
        const size_t c = inside ? (size_t)y * W + x : 0;
        const double v = in[c];
        bool usable = inside && !dm_is_hole(v);
        if (WT) {
            const double w = weight[c];
            usable = usable && w > 0.0 && w <= DBL_MAX;         // (a NaN weight fails both)
            Ws[l] = usable ? w : 0.0;
        }
        Ks[l] = usable ? med_key(v) : MED_SENT;
    }
    __syncthreads();

    for (int l = threadIdx.x; l < T * T; l += MED_THREADS) {
        const int ty = l >> ts, tx = l & (T - 1);
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const size_t c = (size_t)y * W + x;
        const double xc = in[c];
        double res = xc;
        if (!dm_is_hole(xc) || fill) {
            const int ctr = (ty + r) * LW + tx + r;
            uint64_t key;
            bool found;
            if constexpr (R != 0) {
                const MedWinReg<WT, R> win(Ks, Ws, ctr, LW);
                found = med_select<WT>(win, min_count, &key);
            } else {
                const MedWinLds win = {Ks, Ws, ctr, LW, r};
                found = med_select<WT>(win, min_count, &key);
            }
            if (found) res = med_value(key);
        }
        if (changed) {
            const double o = orig[mbase + c];                   // (in place: read before the write below)
            changed[mbase + c] = __double_as_longlong(o) != __double_as_longlong(res) ? 1 : 0;
        }
        out[mbase + c] = res;      // (a copied cell: the double moves unchanged, payload and sign)
    }
}

// ---- host side ------------------------------------------------------------------------------
// false for a shape the entry does not take (the limits of dm_fill_bytes)
static bool med_plan(int32_t M, int32_t H, int32_t W, size_t *plane)
{
    if (!dm_maps_plan(M, H, W, 64 * 65535)) return false;
    *plane = ((size_t)M * H * W * sizeof(double) + 15) & ~(size_t)15;
    return true;
}

// log2 of the tile side (the result does not depend on it).  A tile of 32 has the smaller share
// of halo to stage, which shows only where staging is a visible part of the work: at radius 1
// and 2, whose windows are swept in registers, on a grid of 4096 tiles of 32 or more (16 per
// CU).  Elsewhere a tile of 16 is as fast or faster: it keeps more waves on the CU and fills
// the CUs better on small grids (measured: DESIGN.md 4i).  DM_MEDIAN_TILE = 16 or 32 forces
// one, for measurements and tests.
static int med_tile_shift(int32_t M, int32_t H, int32_t W, int r)
{
    if (const int ts = dm_tile_env("DM_MEDIAN_TILE")) return ts;
    const long long tiles = (long long)((H + 31) >> 5) * ((W + 31) >> 5) * M;
    return r <= 2 && tiles >= 4096 ? 5 : 4;
}

template <int WT, int R>
static hipError_t med_launch(const double *in, const double *weight, int wmaps, int M, int H, int W, int ts, int r,
                             int min_count, int fill, double *out, const double *orig, uint8_t *changed,
                             hipStream_t st)
{
    const int T = 1 << ts;
    const int tiles_x = (W + T - 1) >> ts, tiles_y = (H + T - 1) >> ts;      // tiles_x tiles_y < 2^24
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, M);
    k_median<WT, R><<<grid, MED_THREADS, med_lds(WT, T, r), st>>>(in, weight, wmaps, H, W, tiles_x, ts, r,
                                                                 min_count, fill, out, orig, changed);
    return hipGetLastError();
}

extern "C" {

size_t dm_median_bytes(int32_t M, int32_t H, int32_t W)
{
    size_t plane;
    return med_plan(M, H, W, &plane) ? 2 * plane : 0;
}

int dm_median_filter(const double *d_in, const double *d_weight, int32_t weight_maps, int32_t M, int32_t H,
                     int32_t W, int32_t radius, int32_t min_count, int32_t iters, int32_t flags, double *d_out,
                     uint8_t *d_changed, void *d_work, void *stream)
{
    if (!d_in || !d_out || !d_work) return dm_fail(DM_ERR_ARG, "null input / output / workspace pointer");
    if (M < 1 || H < 1 || W < 1) return dm_fail(DM_ERR_ARG, "bad median shape M=%d H=%d W=%d", M, H, W);
    if (radius < 1 || radius > MED_RMAX) return dm_fail(DM_ERR_ARG, "radius must be in [1, %d] (got %d)", MED_RMAX, radius);
    if (iters < 1 || iters > 64) return dm_fail(DM_ERR_ARG, "iters must be in [1, 64] (got %d)", iters);
    const int K = (2 * radius + 1) * (2 * radius + 1);
    if (min_count < 1 || min_count > K) return dm_fail(DM_ERR_ARG, "min_count must be in [1, %d] (got %d)", K, min_count);
    if (flags & ~DM_MEDIAN_FILL) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    if (d_weight && weight_maps != 1 && weight_maps != M)
        return dm_fail(DM_ERR_ARG, "weight_maps must be 1 or M=%d (got %d)", M, weight_maps);
    size_t plane;
    if (!med_plan(M, H, W, &plane))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "median filter of %d maps of %d x %d cells (at most 65535 maps of 2^31 - 1 cells)", M, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int wt = d_weight ? 1 : 0;
    const int ts = med_tile_shift(M, H, W, radius);
    const int fill = (flags & DM_MEDIAN_FILL) ? 1 : 0;
    double *work0 = (double *)d_work, *work1 = (double *)((char *)d_work + plane);
    const bool inplace = d_in == d_out;
    const double *src = d_in;
    if (inplace && iters == 1) {      // the pass would read what it writes
        DM_HIP_TRY(hipMemcpyAsync(work0, d_in, (size_t)M * H * W * sizeof(double), hipMemcpyDeviceToDevice, st));
        src = work0;
    }
    const double *orig = src;         // holds the input's bits until the last pass has read them
    for (int p = 0; p < iters; ++p) {
        const bool last = p == iters - 1;
        double *dst;
        if (last) dst = d_out;
        else if (inplace) dst = (p & 1) ? work1 : work0;
        else dst = ((iters - 1 - p) & 1) ? work0 : d_out;      // an even number of passes follow: d_out
        const double *og = last && d_changed ? orig : nullptr;
        uint8_t *ch = last ? d_changed : nullptr;
        hipError_t e;
#define MED_GO(WT_, R_) e = med_launch<WT_, R_>(src, d_weight, weight_maps, M, H, W, ts, radius, min_count, fill, dst, og, ch, st)
        if (wt) {
            if (radius == 1) MED_GO(1, 1);
            else if (radius == 2) MED_GO(1, 2);
            else MED_GO(1, 0);
        } else {
            if (radius == 1) MED_GO(0, 1);
            else if (radius == 2) MED_GO(0, 2);
            else if (radius == 3) MED_GO(0, 3);
            else MED_GO(0, 0);
        }
#undef MED_GO
        DM_HIP_TRY(e);
        src = dst;
    }
    return DM_OK;
}

} // extern "C"
