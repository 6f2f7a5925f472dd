// dm_sgm.hip -- gfx950 kernels + C ABI of the semi-global re-matching of a disparity map
// (dm_sgm_refine, include/dmstereo_sgm.h): the quantised ZNCC costs of the (2s+1)^2 integer
// candidates of every cell and a smoothness term between neighbouring cells are minimised along 4
// or 8 scan directions; the sums of the path costs pick the winner of a cell.
//
// Three launches and one memset (of the sums) per call, over a workspace laid out as
//   base  int64 [2][H W]   the base displacement (by - cy, bx - cx) of a cell
//   S     uint32 [H W][L]  the sums of the path costs, L = (2s+1)^2
//   C     uint16 [H W][L]  the costs
//   state uint8 [H W]      dead / fixed / free
// (the bases are int64: by - cy reaches 2^31 where the offset and the disparity are both at their
// limits, and rule 3 needs the exact distance of two displacements).
//
// k_sgm_cost<ND, S>: one thread per cell, workgroups of 32 x 8 cells.  This is k_refine's walk
// (dm_photo_refine.hip) with one img2 window per candidate instead of four: the 2s+1 candidates of
// a candidate row share one walk over the 2r+1 image rows by+ay-r .. by+ay+r, each read once as
// unaligned dwords from the first column any scored candidate needs to the last and cut into the
// shifted rows by funnel shifts; per image row and shift the walk adds W.1, W.W and a.W as chains
// of v_dot4_u32_u8: 3 chains per shift where k_refine has 9 K - 4 per row.  The candidate rows and
// columns are clamped to the scored ones before anything is read, so no byte outside an image row
// is touched: the first column read is bx+axlo-r >= 0, the last bx+axhi+r <= Wi-2, and a row of 3
// bytes (r = 1, one candidate) is read byte by byte.  Every sum stays below 225 * 255^2 < 2^24.
//
// k_sgm_path<S>: one wavefront per scan line and direction, all directions in one launch.  Lane
// a < L (L <= 49) keeps L_rho(., a) of the previous cell in a register and walks the line.  Label b
// of the previous cell has the displacement of label a of this cell iff b = a + (base_p - base_q),
// a shift that is uniform over the wave; so the distance-0 and distance-1 terms are nine
// ds_bpermute lookups of the previous cell's values around a + shift, bounds-checked against the
// window, and the p2 term is one wave-wide minimum (every label at distance 0 or 1 is also met
// with its smaller penalty, so the minimum over all labels plus p2 gives rule 3's minimum).  The
// cell's state, base and costs of the next step are loaded before the current one is finished:
// they do not depend on the chain.  Each lane adds its L into S with an integer atomicAdd: the
// order of the directions does not change an integer sum.
//
// k_sgm_pick: one thread per cell: rule 4's ordered scan over S, rule 5's outputs.  The winner's
// score is computed again from the two windows (the same exact sums, the same float64 tail as in
// k_sgm_cost), so no score is stored per candidate.  A cell reads its own d_row / d_col before it
// writes, and everything else it needs is in the workspace: the outputs may alias the inputs.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include "dm_photo.h"
#include "../../include/dmstereo_sgm.h"

#define SGM_SMAX 3
#define SGM_POSMAX 1073741824.0      // 2^30
#define SGM_PMAX 16384
#define SGM_UNSCORED 2048
#define SGM_ANCHOR 32768
#define SGM_WAVES 4                  // wavefronts of a k_sgm_path workgroup

enum { SGM_DEAD = 0, SGM_FIXED = 1, SGM_FREE = 2 };

__device__ __forceinline__ int sgm_cost_of(double score) { return (int)rint((1.0 - score) * 1024.0); }

// grid: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells.  ND = (r + 2) / 2 dwords per window row.
template <int ND, int S>
__global__ __launch_bounds__(PHO_TX *PHO_TY) void k_sgm_cost(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                            size_t stride2, int Hi, int Wi, const double *d_row,
                                                            const double *d_col, int H, int W, int tiles_x, int oy,
                                                            int ox, int r, const uint8_t *mask, int64_t *base,
                                                            uint16_t *C, uint8_t *state)
{
    constexpr int NC = 2 * S + 1, L = NC * NC;
    constexpr int NW = ND + (2 * S + 3) / 4;       // dwords of the widest row read: 4 ND + 2 S bytes
    int y, x;
    if (!pho_cell(tiles_x, H, W, y, x)) return;
    const size_t HW = (size_t)H * W, c = (size_t)y * W + x;
    const double dr = d_row[c], dc = d_col[c];
    const int cy = y + oy, cx = x + ox;
    bool live = pho_finite(dr) && pho_finite(dc);
    double py = 0.0, px = 0.0;
    if (live) {
        py = (double)cy - dr, px = (double)cx - dc;
        // the test is made in double: only a position it passed is converted
        live = py >= -SGM_POSMAX && py <= SGM_POSMAX && px >= -SGM_POSMAX && px <= SGM_POSMAX;
    }
    if (!live) {
        state[c] = SGM_DEAD;
        return;
    }
    const int by = (int)rint(py), bx = (int)rint(px);      // |by|, |bx| <= 2^30
    base[c] = (int64_t)by - cy;
    base[HW + c] = (int64_t)bx - cx;
    uint16_t *Cc = C + c * L;
    if (mask && mask[c] == 0) {
        state[c] = SGM_FIXED;
#pragma unroll
        for (int k = 0; k < L; ++k) Cc[k] = (uint16_t)(k == S * NC + S ? 0 : SGM_ANCHOR);
        return;
    }
    state[c] = SGM_FREE;
    // the scored candidates: r <= by + ay <= Hi - r - 2, r <= bx + ax <= Wi - r - 2 (no overflow: Hi, Wi <= 2^30)
    const int aylo = max(-S, r - by), ayhi = min(S, Hi - r - 2 - by);
    const int axlo = max(-S, r - bx), axhi = min(S, Wi - r - 2 - bx);
    const bool win1 = cy >= r && cy <= Hi - 1 - r && cx >= r && cx <= Wi - 1 - r;
    if (!win1 || aylo > ayhi || axlo > axhi) {
#pragma unroll
        for (int k = 0; k < L; ++k) Cc[k] = (uint16_t)SGM_UNSCORED;
        return;
    }
    const int D = 2 * r + 1;
    const int64_t n = (int64_t)D * D;
    const int ncand = axhi - axlo + 1;           // candidates of a row: 1 .. NC
    const int nbytes = ncand + D - 1;            // bytes of an image row that they need: >= 3
    uint32_t wmask[ND], sa, saa;
    pho_wmask<ND>(D, wmask);
    const uint8_t *pa = img1 + (size_t)(cy - r) * stride1 + (cx - r);
    pho_moments1<ND>(pa, stride1, D, wmask, sa, saa);
    const int64_t Sa = sa;
    const double VA = (double)(n * (int64_t)saa - Sa * Sa);
    for (int ay = -S; ay <= S; ++ay) {
        uint16_t *Cr = Cc + (ay + S) * NC;
        if (ay < aylo || ay > ayhi) {
#pragma unroll
            for (int k = 0; k < NC; ++k) Cr[k] = (uint16_t)SGM_UNSCORED;
            continue;
        }
        const uint8_t *pb = img2 + (size_t)(by + ay - r) * stride2 + (bx + axlo - r);
        uint32_t St[NC], Qt[NC], At[NC];      // per shift: sum P, sum P^2, sum A P
#pragma unroll
        for (int j = 0; j < NC; ++j) St[j] = Qt[j] = At[j] = 0;
        for (int q = 0; q < D; ++q) {
            uint32_t raw[NW], ac[ND];
            pho_rowz<NW, true>(pb + (size_t)q * stride2, nbytes, raw);
            pho_row<ND>(pa + (size_t)q * stride1, D, ac);
#pragma unroll
            for (int k = 0; k < ND; ++k) ac[k] &= wmask[k];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                uint32_t w[ND];
#pragma unroll
                for (int k = 0; k < ND; ++k) {
                    const int b = j + 4 * k, qd = b >> 2, rm = b & 3;      // compile-time after unrolling
                    const uint32_t lo = qd < NW ? raw[qd < NW ? qd : 0] : 0u;
                    const uint32_t hi = qd + 1 < NW ? raw[qd + 1 < NW ? qd + 1 : 0] : 0u;
                    w[k] = (rm ? ((lo >> (8 * rm)) | (hi << (32 - 8 * rm))) : lo) & wmask[k];
                }
                St[j] = pho_sum<ND>(w, St[j]);
                Qt[j] = pho_dot<ND>(w, w, Qt[j]);
                At[j] = pho_dot<ND>(ac, w, At[j]);
            }
        }
        // shift j of the walk is the candidate ax = axlo + j
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (j < ncand) {
                const int64_t Sp = St[j];
                const double CA = (double)(n * (int64_t)At[j] - Sa * Sp), CB = (double)(n * (int64_t)Qt[j] - Sp * Sp);
                Cr[axlo + S + j] = (uint16_t)sgm_cost_of(pho_zncc(VA, CA, CB));
            }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if (k < axlo + S || k > axhi + S) Cr[k] = (uint16_t)SGM_UNSCORED;
    }
}

// the scan lines of a call: direction d < ndir owns the wavefronts first[d] .. first[d + 1]; total = first[ndir]
struct SgmLines {
    int ndir, total;
    int first[9];
};

__device__ __forceinline__ int sgm_wave_min(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}

// grid: ceil(lines / SGM_WAVES) workgroups of SGM_WAVES wavefronts, one scan line each
template <int S>
__global__ __launch_bounds__(64 * SGM_WAVES) void k_sgm_path(const int64_t *base, const uint16_t *C,
                                                            const uint8_t *state, uint32_t *Ssum, int H, int W, int p1,
                                                            int p2, SgmLines lines)
{
    constexpr int NC = 2 * S + 1, L = NC * NC;
    const int lane = (int)(threadIdx.x & 63);
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SGM_WAVES + (threadIdx.x >> 6)));
    if (wave >= lines.total) return;
    int d = 0, f = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (k < lines.ndir && wave >= lines.first[k]) d = k, f = lines.first[k];
    const int i = wave - f;      // the line of direction d
    // rule 3's order: (0,1) (0,-1) (1,0) (-1,0) (1,1) (1,-1) (-1,1) (-1,-1)
    const int ry = d < 2 ? 0 : (d == 2 || d == 4 || d == 5) ? 1 : -1;
    const int rx = (d == 2 || d == 3) ? 0 : (d == 0 || d == 4 || d == 6) ? 1 : -1;
    // the line's first cell (its predecessor is outside the map) and its length
    int y0, x0, len;
    if (ry == 0) {
        y0 = i, x0 = rx > 0 ? 0 : W - 1, len = W;
    } else if (rx == 0) {
        y0 = ry > 0 ? 0 : H - 1, x0 = i, len = H;
    } else {
        if (i < W) {
            y0 = ry > 0 ? 0 : H - 1, x0 = i;
        } else {
            const int k = i - W + 1;      // 1 .. H - 1
            y0 = ry > 0 ? k : H - 1 - k, x0 = rx > 0 ? 0 : W - 1;
        }
        len = min(ry > 0 ? H - y0 : y0 + 1, rx > 0 ? W - x0 : x0 + 1);
    }
    const size_t HW = (size_t)H * W;
    const ptrdiff_t step = (ptrdiff_t)ry * W + rx;
    const bool act = lane < L;
    const int ay = lane / NC - S, ax = lane % NC - S;
    size_t c = (size_t)y0 * W + x0;
    int st = state[c], cost = act ? (int)C[c * L + lane] : 0;
    int64_t by = base[c], bx = base[HW + c];
    int Lp = 0;
    int64_t pby = 0, pbx = 0;
    bool prev = false;
    for (int t = 0; t < len; ++t) {
        // the next step's inputs: they do not depend on this one (a dead cell's base and costs are never used)
        const size_t cn = t + 1 < len ? (size_t)((ptrdiff_t)c + step) : c;
        const int st_n = state[cn], cost_n = act ? (int)C[cn * L + lane] : 0;
        const int64_t by_n = base[cn], bx_n = base[HW + cn];
        if (st != SGM_DEAD) {
            int Lc = cost;
            if (prev) {
                const int mn = sgm_wave_min(act ? Lp : INT_MAX);
                int best = mn + p2;
                const int64_t ddy = by - pby, ddx = bx - pbx;      // label a here is label a + (ddy, ddx) there
                if (ddy >= -NC && ddy <= NC && ddx >= -NC && ddx <= NC) {
                    const int qy0 = ay + (int)ddy, qx0 = ax + (int)ddx;
#pragma unroll
                    for (int ey = -1; ey <= 1; ++ey) {
#pragma unroll
                        for (int ex = -1; ex <= 1; ++ex) {
                            const int qy = qy0 + ey, qx = qx0 + ex;
                            const bool in = qy >= -S && qy <= S && qx >= -S && qx <= S;
                            const int v = __shfl(Lp, in ? (qy + S) * NC + (qx + S) : 0, 64);
                            if (in) best = min(best, v + ((ey | ex) ? p1 : 0));
                        }
                    }
                }
                Lc = cost + best - mn;
            }
            if (act) atomicAdd(&Ssum[c * L + lane], (uint32_t)Lc);
            Lp = Lc, pby = by, pbx = bx, prev = true;
        } else {
            prev = false;
        }
        c = cn, st = st_n, cost = cost_n, by = by_n, bx = bx_n;
    }
}

// dm_sgm_refine's rule 2 for one candidate: the img1 window around (cy, cx) against the img2 window around (qy, qx)
__device__ __forceinline__ double sgm_score_at(const uint8_t *img1, size_t stride1, const uint8_t *img2, size_t stride2,
                                               int cy, int cx, int qy, int qx, int r)
{
    uint32_t sa = 0, saa = 0, sp = 0, spp = 0, sap = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const uint8_t *ra = img1 + (size_t)(cy + dy) * stride1 + (cx - r);
        const uint8_t *rp = img2 + (size_t)(qy + dy) * stride2 + (qx - r);
        for (int k = 0; k <= 2 * r; ++k) {
            const uint32_t a = ra[k], p = rp[k];
            sa += a, saa += a * a, sp += p, spp += p * p, sap += a * p;
        }
    }
    const int64_t n = (int64_t)(2 * r + 1) * (2 * r + 1), Sa = sa, Sp = sp;
    return pho_zncc((double)(n * (int64_t)saa - Sa * Sa), (double)(n * (int64_t)sap - Sa * Sp),
                    (double)(n * (int64_t)spp - Sp * Sp));
}

// the parabola through the sums (-1, sm), (0, s0), (1, sp): its lowest point, clamped to [-0.5, 0.5]; 0 unless it
// opens upwards
__device__ __forceinline__ double sgm_valley(uint32_t sm, uint32_t s0, uint32_t sp)
{
    const int64_t den = ((int64_t)sm + (int64_t)sp) - 2 * (int64_t)s0;
    if (den <= 0) return 0.0;
    const double t = (0.5 * (double)((int64_t)sm - (int64_t)sp)) / (double)den;
    return t > 0.5 ? 0.5 : (t < -0.5 ? -0.5 : t);
}

// grid: tiles_x * tiles_y workgroups of PHO_TX x PHO_TY cells
__global__ __launch_bounds__(PHO_TX *PHO_TY) void k_sgm_pick(const uint8_t *img1, size_t stride1, const uint8_t *img2,
                                                            size_t stride2, int Hi, int Wi, const double *d_row,
                                                            const double *d_col, int H, int W, int tiles_x, int oy,
                                                            int ox, int r, int S, int subpix, const int64_t *base,
                                                            const uint32_t *Ssum, const uint8_t *state, double *out_row,
                                                            double *out_col, double *score, int8_t *shift)
{
    const int NC = 2 * S + 1, L = NC * NC;
    int y, x;
    if (!pho_cell(tiles_x, H, W, y, x)) return;
    const size_t HW = (size_t)H * W, c = (size_t)y * W + x;
    const double dr = d_row[c], dc = d_col[c];
    double o_row = dr, o_col = dc, o_score = dm_nan();
    int o_ay = 0, o_ax = 0;
    const int cy = y + oy, cx = x + ox;
    if (state[c] == SGM_FREE && cy >= r && cy <= Hi - 1 - r && cx >= r && cx <= Wi - 1 - r) {
        const int by = (int)(base[c] + cy), bx = (int)(base[HW + c] + cx);      // |by|, |bx| <= 2^30
        const int aylo = max(-S, r - by), ayhi = min(S, Hi - r - 2 - by);
        const int axlo = max(-S, r - bx), axhi = min(S, Wi - r - 2 - bx);
        if (aylo <= ayhi && axlo <= axhi) {
            const uint32_t *Sc = Ssum + c * L;
            // the scan runs ay, then ax upwards: among equal sums and distances the first one met stays
            uint32_t best = 0;
            int bay = 0, bax = 0, bd2 = 0;
            bool any = false;
            for (int ay = aylo; ay <= ayhi; ++ay)
                for (int ax = axlo; ax <= axhi; ++ax) {
                    const uint32_t s = Sc[(ay + S) * NC + (ax + S)];
                    const int d2 = ay * ay + ax * ax;
                    if (!any || s < best || (s == best && d2 < bd2)) best = s, bay = ay, bax = ax, bd2 = d2, any = true;
                }
            o_score = sgm_score_at(img1, stride1, img2, stride2, cy, cx, by + bay, bx + bax, r);
            if (bay != 0 || bax != 0) {
                double ty = 0.0, tx = 0.0;
                if (subpix) {
                    const int k = (bay + S) * NC + (bax + S);
                    if (bay - 1 >= aylo && bay + 1 <= ayhi) ty = sgm_valley(Sc[k - NC], best, Sc[k + NC]);
                    if (bax - 1 >= axlo && bax + 1 <= axhi) tx = sgm_valley(Sc[k - 1], best, Sc[k + 1]);
                }
                o_row = (double)((int64_t)cy - by - bay) - ty;
                o_col = (double)((int64_t)cx - bx - bax) - tx;
                o_ay = bay, o_ax = bax;
            }
        }
    }
    out_row[c] = o_row;
    out_col[c] = o_col;
    if (score) score[c] = o_score;
    if (shift) {
        shift[c] = (int8_t)o_ay;
        shift[HW + c] = (int8_t)o_ax;
    }
}

// ---- host side ------------------------------------------------------------------------------
// the workspace of H x W cells with L labels: bases, sums, costs, states; 0 when it does not fit size_t
static size_t sgm_bytes(int32_t H, int32_t W, int32_t search, int32_t paths)
{
    if (search < 1 || search > SGM_SMAX || (paths != 4 && paths != 8)) return 0;
    if (!pho_pair_plan(1, 1, H, W)) return 0;      // (the map's side of the limits: this size has no image)
    const size_t L = (size_t)(2 * search + 1) * (2 * search + 1), per = 16 + 6 * L + 1, HW = (size_t)H * (size_t)W;
    if (HW > (SIZE_MAX - 15) / per) return 0;      // checked before multiplying
    return (HW * per + 15) & ~(size_t)15;
}

extern "C" {

size_t dm_sgm_bytes(int32_t H, int32_t W, int32_t search, int32_t paths) { return sgm_bytes(H, W, search, paths); }

int dm_sgm_refine(const uint8_t *d_img1, int64_t stride1, const uint8_t *d_img2, int64_t stride2, int32_t Hi, int32_t Wi,
                  const double *d_row, const double *d_col, int32_t H, int32_t W, int32_t oy, int32_t ox, int32_t radius,
                  int32_t search, int32_t paths, int32_t p1, int32_t p2, int32_t flags, const uint8_t *d_mask,
                  double *d_out_row, double *d_out_col, double *d_score, int8_t *d_shift, void *d_work, void *stream)
{
    if (!d_img1 || !d_img2 || !d_row || !d_col || !d_out_row || !d_out_col || !d_work)
        return dm_fail(DM_ERR_ARG, "null image / disparity / output / workspace pointer");
    if (const int bad = pho_pair_args(stride1, stride2, Hi, Wi, H, W, oy, ox, radius)) return bad;
    if (search < 1 || search > SGM_SMAX) return dm_fail(DM_ERR_ARG, "search must be in [1, %d] (got %d)", SGM_SMAX, search);
    if (paths != 4 && paths != 8) return dm_fail(DM_ERR_ARG, "paths must be 4 or 8 (got %d)", paths);
    if (p1 < 0 || p1 > p2 || p2 > SGM_PMAX)
        return dm_fail(DM_ERR_ARG, "penalties must satisfy 0 <= p1 <= p2 <= %d (got %d, %d)", SGM_PMAX, p1, p2);
    if (flags & ~DM_SGM_SUBPIX) return dm_fail(DM_ERR_ARG, "unknown flags 0x%x", flags);
    const size_t bytes = sgm_bytes(H, W, search, paths);
    if (!bytes || !pho_pair_plan(Hi, Wi, H, W))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "sgm refine of %d x %d cells on a %d x %d image (at most 2^31 - 1 cells, 2^30 pixels a side)", H, W,
                     Hi, Wi);
    const size_t HW = (size_t)H * W, L = (size_t)(2 * search + 1) * (2 * search + 1);
    int64_t *base = (int64_t *)d_work;
    uint32_t *Ssum = (uint32_t *)((char *)d_work + 16 * HW);
    uint16_t *C = (uint16_t *)((char *)d_work + (16 + 4 * L) * HW);
    uint8_t *state = (uint8_t *)d_work + (16 + 6 * L) * HW;
    int tiles_x;
    const dim3 grid = pho_grid(H, W, &tiles_x);
    hipStream_t st = (hipStream_t)stream;
    DM_HIP_TRY(hipMemsetAsync(Ssum, 0, 4 * L * HW, st));
#define SGM_COST(ND_, S_)                                                                                                \
    k_sgm_cost<ND_, S_><<<grid, PHO_TX * PHO_TY, 0, st>>>(d_img1, (size_t)stride1, d_img2, (size_t)stride2, Hi, Wi, d_row, \
                                                          d_col, H, W, tiles_x, oy, ox, radius, d_mask, base, C, state)
#define SGM_COST_S(ND_)                                                                                                  \
    switch (search) {                                                                                                    \
    case 1: SGM_COST(ND_, 1); break;                                                                                     \
    case 2: SGM_COST(ND_, 2); break;                                                                                     \
    default: SGM_COST(ND_, 3); break;                                                                                    \
    }
    PHO_SWITCH_ND(radius, SGM_COST_S)
#undef SGM_COST_S
#undef SGM_COST
    DM_HIP_TRY(hipGetLastError());
    // the scan lines: H per horizontal direction, W per vertical one, H + W - 1 per diagonal one (H, W <= 64 * 65535:
    // at most 6 (H + W) < 2^31 lines)
    SgmLines lines;
    lines.ndir = paths;
    lines.first[0] = 0;
    for (int d = 0; d < 8; ++d) {
        const int nl = d >= paths ? 0 : d < 2 ? H : d < 4 ? W : H + W - 1;
        lines.first[d + 1] = lines.first[d] + nl;
    }
    lines.total = lines.first[paths];
    const dim3 pgrid((unsigned)((lines.total + SGM_WAVES - 1) / SGM_WAVES));
    switch (search) {
    case 1: k_sgm_path<1><<<pgrid, 64 * SGM_WAVES, 0, st>>>(base, C, state, Ssum, H, W, p1, p2, lines); break;
    case 2: k_sgm_path<2><<<pgrid, 64 * SGM_WAVES, 0, st>>>(base, C, state, Ssum, H, W, p1, p2, lines); break;
    default: k_sgm_path<3><<<pgrid, 64 * SGM_WAVES, 0, st>>>(base, C, state, Ssum, H, W, p1, p2, lines); break;
    }
    DM_HIP_TRY(hipGetLastError());
    k_sgm_pick<<<grid, PHO_TX * PHO_TY, 0, st>>>(d_img1, (size_t)stride1, d_img2, (size_t)stride2, Hi, Wi, d_row, d_col, H,
                                                 W, tiles_x, oy, ox, radius, search, (flags & DM_SGM_SUBPIX) ? 1 : 0, base,
                                                 Ssum, state, d_out_row, d_out_col, d_score, d_shift);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
