// dm_prior.hip -- gfx950 kernels + C ABI of the disparity priors: dm_downsample2, dm_tile_prior,
// dm_pack_plan / dm_pack_tiles and dm_shift_matches (include/dmstereo.h has the definitions).
//
// Every tile of the solver is cut at one origin in img1 and img2, so a match outside a cell's own
// tile of img2 cannot be found.  With an expected disparity q_t per tile the img2 crop is cut at
// o_t - q_t instead.  The level, pyramid and matching kernels stay as they are: a tile's result
// depends only on its own two crops, so the offset crops are copied side by side into a fresh
// image pair (dm_pack_tiles) which the unchanged kernels solve at the grid's origins, and the
// matches are moved back into the frame of img1's tile afterwards (dm_shift_matches).  The
// expectation comes from a map of the same pair (dm_tile_prior), for instance one solved at half
// the resolution (dm_downsample2).  All four are memory bound and tiny next to the solve.
//
// k_downsample2<VEC>   VEC: a thread reads 2 x 32 source bytes as four 16-byte loads and writes 16
//                      destination bytes in one store (pointers and strides multiples of 16, W/2 a
//                      multiple of 16); else one thread per destination byte.
// k_tile_prior         one workgroup of 1024 threads per tile.  The lower median of a plane is
//                      selected by the order-preserving key of the double (dm_median.hip's) with a
//                      radix select, 8 bits a sweep from the top: 8 sweeps of the footprint, both
//                      planes in one sweep, each counting into 256 LDS bins per plane with integer
//                      atomics and closed by a wave that picks the bin of the wanted rank.  The
//                      counts are exact, so the result does not depend on the schedule.  (A first
//                      version counted one bit a sweep, 64 sweeps each closed by a reduction over
//                      the workgroup: engine.tile_prior took 0.44 ms for the 64 tiles of a 1024^2
//                      pair at S = 128, scale 2, against 0.05 ms now.)
// k_prior_fallback     one workgroup: a bit-by-bit selection over the int32 priors of the tiles
//                      that measured one, written to those that did not; it returns at once when
//                      every tile measured its own.
// k_pack_tiles         a thread writes 16 bytes of a packed row in one store (the packed pitch is
//                      a multiple of 16); the source crops start at any byte, so it gathers them
//                      byte by byte.  grid.y = 2: the two images.
// k_shift_matches<VEC> VEC (h0 w0 even, pointer a multiple of 16): two doubles per thread.
#include <hip/hip_runtime.h>

#include "dm_host.h"      // dm_fail, DM_HIP_TRY, dm_is_hole

#define PRI_THREADS 256
#define PRI_WAVES (PRI_THREADS / 64)
#define PRI_TP_THREADS 1024      // k_tile_prior: a footprint of S^2 / 4 cells in a few sweeps
#define PRI_SIGN 0x8000000000000000ULL
#define PRI_QMAX 1073741824.0      // 2^30: |q| is clamped to it before the conversion to int32
#define PRI_SIDE_MAX (1 << 30)

__device__ __forceinline__ uint64_t pri_key(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return (b & PRI_SIGN) ? ~b : (b | PRI_SIGN);
}

__device__ __forceinline__ double pri_value(uint64_t k)
{
    return __longlong_as_double((long long)((k & PRI_SIGN) ? (k ^ PRI_SIGN) : ~k));
}

// the sums of a and b over the workgroup, in every thread (red: 2 * PRI_WAVES ints of LDS)
__device__ __forceinline__ void pri_sum2(int &a, int &b, int *red)
{
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();      // the previous round's reads of red are done
    if ((threadIdx.x & 63) == 0) {
        red[2 * wave] = a;
        red[2 * wave + 1] = b;
    }
    __syncthreads();
    a = b = 0;
    for (int w = 0; w < PRI_WAVES; ++w) {
        a += red[2 * w];
        b += red[2 * w + 1];
    }
}

// ---- dm_downsample2 -------------------------------------------------------------------------
__device__ __forceinline__ unsigned ds_quad(unsigned top, unsigned bot, int k)      // bytes 2k, 2k + 1 of both words
{
    const unsigned s = 16 * k;
    return (((top >> s) & 0xffu) + ((top >> (s + 8)) & 0xffu) + ((bot >> s) & 0xffu) + ((bot >> (s + 8)) & 0xffu) + 2u) >> 2;
}

template <int VEC>
__global__ __launch_bounds__(PRI_THREADS) void k_downsample2(const uint8_t *src, size_t sstride, int Hd, int Wd,
                                                            uint8_t *dst, size_t dstride)
{
    const size_t idx = blockIdx.x * (size_t)PRI_THREADS + threadIdx.x;
    if (VEC) {
        const int chunks = Wd >> 4;      // Wd % 16 == 0
        if (idx >= (size_t)Hd * chunks) return;
        const int y = (int)(idx / chunks), c = (int)(idx - (size_t)y * chunks);
        const uint4 *r0 = (const uint4 *)(src + (size_t)(2 * y) * sstride + 32 * (size_t)c);
        const uint4 *r1 = (const uint4 *)(src + (size_t)(2 * y + 1) * sstride + 32 * (size_t)c);
        const uint4 a0 = r0[0], a1 = r0[1], b0 = r1[0], b1 = r1[1];
        const unsigned top[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const unsigned bot[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        unsigned o[4];
#pragma unroll
        for (int w = 0; w < 4; ++w)      // a source word gives two destination bytes
            o[w] = ds_quad(top[2 * w], bot[2 * w], 0) | (ds_quad(top[2 * w], bot[2 * w], 1) << 8) |
                   (ds_quad(top[2 * w + 1], bot[2 * w + 1], 0) << 16) | (ds_quad(top[2 * w + 1], bot[2 * w + 1], 1) << 24);
        *(uint4 *)(dst + (size_t)y * dstride + 16 * (size_t)c) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        if (idx >= (size_t)Hd * Wd) return;
        const int y = (int)(idx / Wd), x = (int)(idx - (size_t)y * Wd);
        const uint8_t *r0 = src + (size_t)(2 * y) * sstride + 2 * (size_t)x, *r1 = r0 + sstride;
        dst[(size_t)y * dstride + x] = (uint8_t)(((unsigned)r0[0] + r0[1] + r1[0] + r1[1] + 2u) >> 2);
    }
}

// ---- dm_tile_prior --------------------------------------------------------------------------
// the footprint of image pixels [first, first + len - 1] in a coarse map of n cells: [lo, hi]
__device__ __forceinline__ void pri_footprint(int first, int len, int e, int s, int n, int *lo, int *hi)
{
    const int a = first / s - e, b = (first + len - 1) / s - e;      // first >= 0: the division floors
    *lo = min(max(a, 0), n - 1);
    *hi = min(max(b, 0), n - 1);
}

// The bin of a 256-bin histogram that holds the element of rank *r (0-based, *r < the histogram's
// total), found by one wave: lane l sums bins 4 l .. 4 l + 3, an inclusive scan over the lanes finds
// the lane, the lane walks its four bins.  Every lane returns the bin; *r becomes the rank inside
// that bin and *total the histogram's total.
__device__ __forceinline__ int pri_pick_bin(const unsigned *hist, int *r, int *total)
{
    const int lane = threadIdx.x & 63;
    int c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += c[k] = (int)hist[4 * lane + k];
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    *total = __shfl(incl, 63);
    if (*total == 0) return 0;
    const int first = __ffsll((long long)__ballot(incl > *r)) - 1;      // the first lane whose bins reach past the rank
    int bin = 0, rest = 0;
    if (lane == first) {
        rest = *r - (incl - sum);
        int k = 0;
        while (k < 3 && rest >= c[k]) rest -= c[k++];
        bin = 4 * lane + k;
    }
    *r = __shfl(rest, first);
    return __shfl(bin, first);
}

// One workgroup per tile.  A radix select on the key, 8 bits a sweep from the top: a sweep counts,
// per plane, the usable cells whose key has the prefix found so far into 256 LDS bins by their next
// 8 bits (integer atomics: the counts are exact whatever the order), one wave per plane then picks
// the bin that holds the wanted rank.  8 sweeps of the footprint instead of one per bit.
__global__ __launch_bounds__(PRI_TP_THREADS) void k_tile_prior(const double *drow, const double *dcol, int Hc, int Wc,
                                                              const int32_t *org, int h0, int w0, int e, int s,
                                                              int32_t *q, uint8_t *valid)
{
    __shared__ unsigned hist[2][256];
    __shared__ uint64_t sh_key[2];
    __shared__ int sh_rank[2], sh_n;
    const int t = blockIdx.x;
    int y0, y1, x0, x1;
    pri_footprint(max(org[2 * t], 0) + e, h0, e, s, Hc, &y0, &y1);
    pri_footprint(max(org[2 * t + 1], 0) + e, w0, e, s, Wc, &x0, &x1);
    const int fw = x1 - x0 + 1, cells = (y1 - y0 + 1) * fw;      // <= h0 w0 < 2^31
    const int wave = threadIdx.x >> 6;

    uint64_t kr = 0, kc = 0;      // the bits of the two medians' keys found so far
    int rank = 0;                 // waves 0 and 1: the wanted rank among the cells with that prefix
    for (int p = 0; p < 8; ++p) {
        const int shift = 56 - 8 * p;
        if (threadIdx.x < 512) hist[threadIdx.x >> 8][threadIdx.x & 255] = 0u;
        __syncthreads();
        for (int l = threadIdx.x; l < cells; l += PRI_TP_THREADS) {
            const size_t c = (size_t)(y0 + l / fw) * Wc + x0 + l % fw;
            const double vr = drow[c], vc = dcol[c];
            if (dm_is_hole(vr) || dm_is_hole(vc)) continue;
            const uint64_t a = pri_key(vr), b = pri_key(vc);
            if (p == 0 || (a >> (shift + 8)) == (kr >> (shift + 8))) atomicAdd(&hist[0][(a >> shift) & 255], 1u);
            if (p == 0 || (b >> (shift + 8)) == (kc >> (shift + 8))) atomicAdd(&hist[1][(b >> shift) & 255], 1u);
        }
        __syncthreads();
        if (wave < 2) {      // wave 0: the row plane, wave 1: the column plane
            int total, r = rank;
            if (p == 0) {      // the first sweep counts every usable cell: n, and the rank of the lower median
                int n = 0;
                for (int k = threadIdx.x & 63; k < 256; k += 64) n += (int)hist[wave][k];
                for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
                r = n > 0 ? (n - 1) >> 1 : 0;
                if (threadIdx.x == 0) sh_n = n;
            }
            const int bin = pri_pick_bin(hist[wave], &r, &total);
            rank = r;
            if ((threadIdx.x & 63) == 0) sh_key[wave] = (wave ? kc : kr) | ((uint64_t)bin << shift);
        }
        __syncthreads();
        if (sh_n == 0) {      // (the whole workgroup) no usable cell: k_prior_fallback fills the prior in
            if (threadIdx.x == 0) {
                q[2 * t] = q[2 * t + 1] = 0;
                valid[t] = 0;
            }
            return;
        }
        kr = sh_key[0];
        kc = sh_key[1];
    }
    if (threadIdx.x == 0) {
        const double mr = rint((double)s * pri_value(kr)), mc = rint((double)s * pri_value(kc));
        q[2 * t] = (int32_t)fmin(fmax(mr, -PRI_QMAX), PRI_QMAX);
        q[2 * t + 1] = (int32_t)fmin(fmax(mc, -PRI_QMAX), PRI_QMAX);
        valid[t] = 1;
    }
}

// one workgroup.  The tiles without a prior of their own take, per component, the lower median of
// the priors of the others (0 if there is none)
__global__ __launch_bounds__(PRI_THREADS) void k_prior_fallback(int32_t *q, const uint8_t *valid, int T)
{
    __shared__ int red[2 * PRI_WAVES];
    int n = 0, unused = 0;
    for (int t = threadIdx.x; t < T; t += PRI_THREADS) n += valid[t] ? 1 : 0;
    pri_sum2(n, unused, red);
    if (n == T) return;
    int32_t fr = 0, fc = 0;
    if (n > 0) {
        const int rank = (n - 1) >> 1;
        uint32_t kr = 0, kc = 0;      // keys: the int32 with its sign bit flipped
        for (int b = 31; b >= 0; --b) {
            const uint32_t cr = kr | (1u << b), cc = kc | (1u << b);
            int nr = 0, nc = 0;
            for (int t = threadIdx.x; t < T; t += PRI_THREADS) {
                const bool u = valid[t] != 0;
                nr += (u && ((uint32_t)q[2 * t] ^ 0x80000000u) < cr) ? 1 : 0;
                nc += (u && ((uint32_t)q[2 * t + 1] ^ 0x80000000u) < cc) ? 1 : 0;
            }
            pri_sum2(nr, nc, red);
            if (nr <= rank) kr = cr;
            if (nc <= rank) kc = cc;
        }
        fr = (int32_t)(kr ^ 0x80000000u);
        fc = (int32_t)(kc ^ 0x80000000u);
    }
    __syncthreads();      // every read of a measured prior precedes the writes (they touch other tiles anyway)
    for (int t = threadIdx.x; t < T; t += PRI_THREADS)
        if (!valid[t]) {
            q[2 * t] = fr;
            q[2 * t + 1] = fc;
        }
}

// ---- dm_pack_tiles --------------------------------------------------------------------------
struct PackPlan {
    int gx, gy, ch, cw, Hp, Wp;
};

// false for a batch the entry does not take
static bool pack_plan(int32_t T, int32_t h0, int32_t w0, int32_t ws, PackPlan *p)
{
    if (T < 1 || h0 < 1 || w0 < 1 || ws < 1) return false;
    const long long ch = (long long)h0 + ws - 1, cw = (long long)w0 + ws - 1;
    if (ch > 65536 || cw > 65536) return false;
    // a grid about as high as it is wide, at most 65536 crops a row
    long long gx = 1;
    while (gx * gx * cw < (long long)T * ch && gx < T) ++gx;
    if (gx > 65536) gx = 65536;
    const long long gy = (T + gx - 1) / gx;
    const long long Hp = gy * ch, Wp = (gx * cw + 15) & ~15LL;
    if (Hp > PRI_SIDE_MAX || Wp > PRI_SIDE_MAX) return false;
    p->gx = (int)gx; p->gy = (int)gy; p->ch = (int)ch; p->cw = (int)cw; p->Hp = (int)Hp; p->Wp = (int)Wp;
    return true;
}

// the crop origin of tile t along one axis in img2 (o - q clamped into [0, dim - size]); img1's
// origin is clamped the same way, which changes nothing for a batch whose crops lie inside the
// image (the caller's check) and keeps every read inside it for one that does not
__device__ __forceinline__ int pack_clamp(long long v, int dim, int size) { return (int)min(max(v, 0LL), (long long)(dim - size)); }

__global__ __launch_bounds__(PRI_THREADS) void k_pack_tiles(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                           size_t stride2, int H, int W, const int32_t *org,
                                                           const int32_t *prior, int T, PackPlan p, uint8_t *pack1,
                                                           uint8_t *pack2, int32_t *pack_org, int32_t *q_eff)
{
    const size_t idx = blockIdx.x * (size_t)PRI_THREADS + threadIdx.x;
    const int second = blockIdx.y;
    if (!second && idx < (size_t)T) {      // the grid origin and the effective prior of tile idx
        const int t = (int)idx;
        const int oy = pack_clamp(org[2 * t], H, p.ch), ox = pack_clamp(org[2 * t + 1], W, p.cw);
        pack_org[2 * t] = (t / p.gx) * p.ch;
        pack_org[2 * t + 1] = (t % p.gx) * p.cw;
        q_eff[2 * t] = oy - pack_clamp((long long)org[2 * t] - prior[2 * t], H, p.ch);
        q_eff[2 * t + 1] = ox - pack_clamp((long long)org[2 * t + 1] - prior[2 * t + 1], W, p.cw);
    }
    const int chunks = p.Wp >> 4;
    if (idx >= (size_t)p.Hp * chunks) return;
    const int y = (int)(idx / chunks), x = (int)(idx - (size_t)y * chunks) << 4;
    const int gyi = y / p.ch, cy = y - gyi * p.ch;
    const uint8_t *img = second ? img2 : img1;
    const size_t stride = second ? stride2 : stride1;
    int gxi = x / p.cw, cx = x - gxi * p.cw;
    const uint8_t *row = nullptr;      // the source row of the crop under x; NULL: no crop there
    auto locate = [&]() {
        const int t = gyi * p.gx + gxi;
        if (gxi >= p.gx || t >= T) {
            row = nullptr;
            return;
        }
        const long long qy = second ? prior[2 * t] : 0, qx = second ? prior[2 * t + 1] : 0;
        const int sy = pack_clamp((long long)org[2 * t] - qy, H, p.ch), sx = pack_clamp((long long)org[2 * t + 1] - qx, W, p.cw);
        row = img + (size_t)(sy + cy) * stride + sx;
    };
    locate();
    unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const unsigned v = row ? row[cx] : 0u;
        o[k >> 2] |= v << (8 * (k & 3));
        if (++cx == p.cw) {
            cx = 0;
            ++gxi;
            locate();
        }
    }
    *(uint4 *)((second ? pack2 : pack1) + (size_t)y * p.Wp + x) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- dm_shift_matches -----------------------------------------------------------------------
// rows 0 and 1 of tile t are its first 2 P doubles
template <int VEC>
__global__ __launch_bounds__(PRI_THREADS) void k_shift_matches(double *match, const int32_t *q_eff, size_t T, size_t P)
{
    const size_t idx = blockIdx.x * (size_t)PRI_THREADS + threadIdx.x;
    const size_t per = VEC ? P : 2 * P;      // threads per tile
    if (idx >= T * per) return;
    const size_t t = idx / per, l = idx - t * per;
    if (VEC) {      // P even: a pair of doubles lies in one row
        double2 *m = (double2 *)(match + t * 3 * P) + l;
        const double q = (double)q_eff[2 * t + (2 * l >= P ? 1 : 0)];
        double2 v = *m;
        v.x -= q;
        v.y -= q;
        *m = v;
    } else {
        match[t * 3 * P + l] -= (double)q_eff[2 * t + (l >= P ? 1 : 0)];
    }
}

static int pri_blocks(unsigned long long n, unsigned *blocks)
{
    const unsigned long long nb = (n + PRI_THREADS - 1) / PRI_THREADS;
    if (nb > 0x7fffffffull) return dm_fail(DM_ERR_UNSUPPORTED, "%llu elements in one launch", n);
    *blocks = (unsigned)nb;
    return DM_OK;
}

static bool pri_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

int dm_downsample2(const uint8_t *d_src, int64_t stride, int32_t H, int32_t W, uint8_t *d_dst, int64_t dst_stride,
                   void *stream)
{
    if (!d_src || !d_dst) return dm_fail(DM_ERR_ARG, "null image pointer");
    if (H < 2 || W < 2) return dm_fail(DM_ERR_ARG, "an image of %d x %d has no 2 x 2 block", H, W);
    const int Hd = H / 2, Wd = W / 2;
    if (stride < W || dst_stride < Wd)
        return dm_fail(DM_ERR_ARG, "row stride below the width (got %lld for %d, %lld for %d)", (long long)stride, W,
                     (long long)dst_stride, Wd);
    const bool vec = Wd % 16 == 0 && pri_al16(d_src) && pri_al16(d_dst) && stride % 16 == 0 && dst_stride % 16 == 0;
    unsigned nb;
    const int rc = pri_blocks((unsigned long long)Hd * (vec ? Wd / 16 : Wd), &nb);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (vec) k_downsample2<1><<<nb, PRI_THREADS, 0, st>>>(d_src, (size_t)stride, Hd, Wd, d_dst, (size_t)dst_stride);
    else k_downsample2<0><<<nb, PRI_THREADS, 0, st>>>(d_src, (size_t)stride, Hd, Wd, d_dst, (size_t)dst_stride);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

int dm_tile_prior(const double *d_row, const double *d_col, int32_t Hc, int32_t Wc, const int32_t *d_origins, int32_t T,
                  int32_t h0, int32_t w0, int32_t e, int32_t scale, int32_t *d_q, uint8_t *d_valid, void *stream)
{
    if (!d_row || !d_col || !d_origins || !d_q || !d_valid) return dm_fail(DM_ERR_ARG, "null plane / origin / output pointer");
    if (Hc < 1 || Wc < 1 || (long long)Hc * Wc > 0x7fffffffLL) return dm_fail(DM_ERR_ARG, "bad map shape Hc=%d Wc=%d", Hc, Wc);
    if (T < 1 || h0 < 1 || w0 < 1 || h0 > 65536 || w0 > 65536 || (long long)h0 * w0 > 0x7fffffffLL)
        return dm_fail(DM_ERR_ARG, "bad tile batch T=%d h0=%d w0=%d", T, h0, w0);
    if (e < 0 || e > 65536) return dm_fail(DM_ERR_ARG, "e must be in [0, 65536] (got %d)", e);
    if (scale != 1 && scale != 2) return dm_fail(DM_ERR_ARG, "scale must be 1 or 2 (got %d)", scale);
    hipStream_t st = (hipStream_t)stream;
    k_tile_prior<<<(unsigned)T, PRI_TP_THREADS, 0, st>>>(d_row, d_col, Hc, Wc, d_origins, h0, w0, e, scale, d_q, d_valid);
    DM_HIP_TRY(hipGetLastError());
    k_prior_fallback<<<1, PRI_THREADS, 0, st>>>(d_q, d_valid, T);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

int dm_pack_plan(int32_t T, int32_t h0, int32_t w0, int32_t ws, int32_t *grid_cols, int32_t *Hp, int32_t *Wp)
{
    PackPlan p;
    if (!grid_cols || !Hp || !Wp) return dm_fail(DM_ERR_ARG, "null output pointer");
    if (!pack_plan(T, h0, w0, ws, &p))
        return dm_fail(DM_ERR_UNSUPPORTED, "packing of %d tiles of %d x %d cells, ws %d", T, h0, w0, ws);
    *grid_cols = p.gx; *Hp = p.Hp; *Wp = p.Wp;
    return DM_OK;
}

int dm_pack_tiles(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t H, int32_t W,
                  const int32_t *d_origins, const int32_t *d_prior, int32_t T, int32_t h0, int32_t w0, int32_t ws,
                  uint8_t *d_pack1, uint8_t *d_pack2, int32_t *d_pack_origins, int32_t *d_q_eff, void *stream)
{
    if (!d_img1 || !d_img2 || !d_origins || !d_prior || !d_pack1 || !d_pack2 || !d_pack_origins || !d_q_eff)
        return dm_fail(DM_ERR_ARG, "null image / origin / prior / output pointer");
    PackPlan p;
    if (!pack_plan(T, h0, w0, ws, &p))
        return dm_fail(DM_ERR_UNSUPPORTED, "packing of %d tiles of %d x %d cells, ws %d", T, h0, w0, ws);
    if (H < p.ch || W < p.cw || H > PRI_SIDE_MAX || W > PRI_SIDE_MAX)
        return dm_fail(DM_ERR_ARG, "an image of %d x %d holds no crop of %d x %d", H, W, p.ch, p.cw);
    if (stride1 < W || stride2 < W)
        return dm_fail(DM_ERR_ARG, "row stride below the image width %d (got %lld, %lld)", W, (long long)stride1,
                     (long long)stride2);
    if (!pri_al16(d_pack1) || !pri_al16(d_pack2)) return dm_fail(DM_ERR_ARG, "the packed images must be 16-byte aligned");
    unsigned nb;
    const unsigned long long chunks = (unsigned long long)p.Hp * (p.Wp / 16);
    const int rc = pri_blocks(chunks > (unsigned long long)T ? chunks : (unsigned long long)T, &nb);
    if (rc) return rc;
    k_pack_tiles<<<dim3(nb, 2), PRI_THREADS, 0, (hipStream_t)stream>>>(d_img1, (size_t)stride1, d_img2, (size_t)stride2, H, W,
                                                                      d_origins, d_prior, T, p, d_pack1, d_pack2,
                                                                      d_pack_origins, d_q_eff);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

int dm_shift_matches(double *d_match, const int32_t *d_q_eff, int32_t T, int32_t h0, int32_t w0, void *stream)
{
    if (!d_match || !d_q_eff) return dm_fail(DM_ERR_ARG, "null match / prior pointer");
    if (T < 1 || h0 < 1 || w0 < 1 || (long long)h0 * w0 > 0x7fffffffLL)
        return dm_fail(DM_ERR_ARG, "bad match shape T=%d h0=%d w0=%d", T, h0, w0);
    const size_t P = (size_t)h0 * w0;
    const bool vec = P % 2 == 0 && pri_al16(d_match);
    unsigned nb;
    const int rc = pri_blocks((unsigned long long)T * (vec ? P : 2 * P), &nb);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (vec) k_shift_matches<1><<<nb, PRI_THREADS, 0, st>>>(d_match, d_q_eff, (size_t)T, P);
    else k_shift_matches<0><<<nb, PRI_THREADS, 0, st>>>(d_match, d_q_eff, (size_t)T, P);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
