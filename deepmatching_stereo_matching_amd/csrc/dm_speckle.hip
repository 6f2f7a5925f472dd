// dm_speckle.hip -- gfx950 kernels + C ABI of the speckle filter: removal of small disparity
// segments (dm_filter_speckles, include/dmstereo.h).
//
// A cell is finite when it passes the range test on the double (NaN, +-inf: holes).  Two finite
// 4-neighbours are joined iff fabs(a - b) <= max_diff (float64, no contraction); a segment is a
// connected component of that graph, its size its cell count, its label the smallest linear
// index i W + j among its cells.  Cells of segments with size <= max_size become NaN, every
// other cell is copied bit for bit.  tests/test_speckle_host.py restates this in plain loops
// (speckle_restate); the kernels equal it bit for bit, whatever the tile side and the schedule.
//
// Labelling is union-find in which a parent is always a smaller-or-equal linear index, so the
// root of a component is its minimum and labels and integer sizes do not depend on the order
// in which unions happen:
//   k_spk_local    one workgroup per tile of T x T cells (T = 64): values and parents in LDS.
//                  Each cell starts under the first cell of its run of joined cells in its row
//                  (one ballot per row, no atomics); then a cell joined with its upper
//                  neighbour unites the two runs by LDS atomicMin, unless the pair to its left
//                  has to do so anyway; the tile is flattened and each cell's parent written
//                  to the global label array as the global index of its local root; sizes
//                  zeroed.
//   k_spk_border   each pair of cells joined across a tile edge unites the two global roots
//                  (unless the previous pair along the edge has to do so anyway):
//                  old = atomicMin(&L[big], small); old != big: go on from (old, small).
//                  Parents are read by agent-scope atomic loads (no stale L1 line is followed).
//   k_spk_count    every cell walks to its root and stores it (no union runs any more); the
//                  counts are reduced per tile in an LDS hash table keyed by root, then one
//                  global integer atomicAdd per (tile, root).
//   k_spk_apply    each cell reads its own input, its label and size[label] and writes d_out
//                  and the optional outputs.  Only this kernel writes d_out and a thread reads
//                  only its own input cell, so d_out may be d_in.
//   k_spk_one      a map of at most one tile: all of the above in one launch, in LDS.
//
// While unions may run, a parent entry is written by atomicMin only (LDS or global), so it only
// ever decreases; plain stores happen in the row step, behind a barrier before the first union,
// and in the flatten steps, after the barrier or the kernel boundary that ends the unions,
// where they store an ancestor of the old parent.  Every loop
// is lock-free and no thread waits for another thread's store: a find follows strictly
// decreasing parents and ends at an index that is its own parent; a union either links
// (old == big), finds both cells under one root, or goes on from a strictly smaller index, and
// indices are bounded below by 0; a hash insert probes at most SPK_SLOTS slots of a table that
// holds at most T T <= SPK_SLOTS / 2 keys.  No grid barrier, no cooperative launch, no flag.
// Integer atomics only.
#include <hip/hip_runtime.h>

#include <math.h>

#include "dm_host.h"      // dm_fail, DM_HIP_TRY, dm_is_hole, dm_nan, dm_maps_plan

#define SPK_TMAX 64                      // largest (and default) tile side; a power of two
#define SPK_THREADS 256
#define SPK_SLOTS 8192                   // slots of k_spk_count's table: 2 SPK_TMAX^2
#define SPK_SLOT_BITS 13

static constexpr size_t SPK_LOCAL_LDS = (size_t)SPK_TMAX * SPK_TMAX * (sizeof(double) + sizeof(int));
static constexpr size_t SPK_ONE_LDS = SPK_LOCAL_LDS + (size_t)SPK_TMAX * SPK_TMAX * sizeof(uint32_t);

// both finite; a difference that overflows to inf is joined only by max_diff = +inf
__device__ __forceinline__ bool spk_joined(double a, double b, double max_diff) { return fabs(a - b) <= max_diff; }

// ---- union-find on the parents of one tile in LDS -------------------------------------------
__device__ __forceinline__ int spk_lfind(int *P, int a)
{
    for (;;) {
        const int p = __hip_atomic_load(&P[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == a) return a;
        a = p;      // p < a
    }
}

__device__ __forceinline__ void spk_lunion(int *P, int a, int b)
{
    for (;;) {
        a = spk_lfind(P, a);
        b = spk_lfind(P, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&P[a], b);      // P[a] = min(P[a], b): it only decreases
        if (old == a) return;                     // a was still a root: linked
        a = old;                                  // somebody linked a first: old < a joins b's side
    }
}

// The tile at (y0, x0) of the map `in` (H x W) into LDS: V [T T] values (cells outside the map
// are holes), P [T T] parents, flattened when this returns (P[l] = the smallest local index of
// l's component inside the tile, -1 for a hole).  T = 1 << ts.  Ends with a barrier.
__device__ __forceinline__ void spk_tile_label(const double *in, int H, int W, int y0, int x0, int ts,
                                               double max_diff, double *V, int *P)
{
    const int T = 1 << ts, cells = T * T;
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        const int y = y0 + (l >> ts), x = x0 + (l & (T - 1));
        const double v = (y < H && x < W) ? in[(size_t)y * W + x] : dm_nan();
        V[l] = v;
    }
    __syncthreads();
    // rows first, without atomics: a row of the tile lies in one wave (T divides 64, SPK_THREADS
    // is a multiple of 64, T T of SPK_THREADS: every lane takes every trip), so the start of a
    // cell's run of joined cells is the last lane at or below its own that is not joined with
    // its left neighbour -- one ballot.  No union runs yet: plain stores.
    const int lane = threadIdx.x & 63;
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        const double v = V[l];
        const bool hole = dm_is_hole(v);
        bool brk = true;
        if (!hole && (l & (T - 1)) > 0) {
            const double u = V[l - 1];
            brk = dm_is_hole(u) || !spk_joined(v, u, max_diff);
        }
        const unsigned long long m = __ballot(brk) & ((2ULL << lane) - 1ULL);      // column 0 always breaks: m != 0
        P[l] = hole ? -1 : l - (lane - (63 - __clzll(m)));
    }
    __syncthreads();
    // then columns: a cell joined with its upper neighbour unites the two runs, unless the pair
    // to its left does so already (both runs reach one cell further left and are joined there)
    for (int l = threadIdx.x + T; l < cells; l += SPK_THREADS) {
        const double v = V[l], u = V[l - T];
        if (dm_is_hole(v) || dm_is_hole(u) || !spk_joined(v, u, max_diff)) continue;
        if ((l & (T - 1)) > 0) {
            const double vl = V[l - 1], ul = V[l - T - 1];
            if (!dm_is_hole(vl) && !dm_is_hole(ul) && spk_joined(v, vl, max_diff) && spk_joined(u, ul, max_diff) &&
                spk_joined(vl, ul, max_diff))
                continue;
        }
        spk_lunion(P, l, l - T);
    }
    __syncthreads();
    // flatten: no union runs any more; a store replaces a parent by one of its ancestors, so a
    // find that reads either value ends at the same root
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        if (dm_is_hole(V[l])) continue;
        const int r = spk_lfind(P, l);
        __hip_atomic_store(&P[l], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
}

// grid (ceil(W / T), ceil(H / T), M).  L [M][H][W] labels, S [M][H][W] sizes by root (zeroed here).
__global__ __launch_bounds__(SPK_THREADS) void k_spk_local(const double *in, int H, int W, int ts, double max_diff,
                                                           int32_t *L, uint32_t *S)
{
    extern __shared__ double spk_lds[];
    const int T = 1 << ts, cells = T * T;
    double *V = spk_lds;
    int *P = (int *)(V + cells);
    const size_t mbase = (size_t)blockIdx.z * H * W;
    const int y0 = blockIdx.y << ts, x0 = blockIdx.x << ts;
    spk_tile_label(in + mbase, H, W, y0, x0, ts, max_diff, V, P);
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        const int y = y0 + (l >> ts), x = x0 + (l & (T - 1));
        if (y >= H || x >= W) continue;
        const int r = P[l];
        const size_t g = mbase + (size_t)y * W + x;
        L[g] = r < 0 ? -1 : (y0 + (r >> ts)) * W + x0 + (r & (T - 1));      // < H W <= 2^31 - 1
        S[g] = 0;
    }
}

// ---- union-find on the global labels of one map ---------------------------------------------
__device__ __forceinline__ int spk_gfind(int32_t *L, int a)
{
    for (;;) {
        const int p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == a) return a;
        a = p;      // p < a
    }
}

__device__ __forceinline__ void spk_gunion(int32_t *L, int a, int b)
{
    for (;;) {
        a = spk_gfind(L, a);
        b = spk_gfind(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// The pairs across the left and the upper edge of each tile.  grid as k_spk_local, 2 SPK_TMAX
// threads: thread t < T takes row y0 + t of the left edge, thread T + t column x0 + t of the
// upper edge.
__global__ __launch_bounds__(2 * SPK_TMAX) void k_spk_border(const double *in, int H, int W, int ts, double max_diff,
                                                             int32_t *L)
{
    const int T = 1 << ts;
    const size_t mbase = (size_t)blockIdx.z * H * W;
    in += mbase;
    L += mbase;
    const int y0 = blockIdx.y << ts, x0 = blockIdx.x << ts;
    const int t = threadIdx.x;
    int a, b, back;      // linear indices of the pair, b the cell of the neighbouring tile; the step
    bool first;          // back to the previous pair along the edge, if this tile has one
    if (t < T) {
        if (x0 == 0 || y0 + t >= H) return;
        a = (y0 + t) * W + x0;
        b = a - 1;
        back = W;
        first = t == 0;
    } else if (t < 2 * T) {
        if (y0 == 0 || x0 + (t - T) >= W) return;
        a = y0 * W + x0 + (t - T);
        b = a - W;
        back = 1;
        first = t == T;
    } else {
        return;
    }
    const double va = in[a], vb = in[b];
    if (dm_is_hole(va) || dm_is_hole(vb) || !spk_joined(va, vb, max_diff)) return;
    if (!first) {
        // the previous pair along the edge does this union already when it is joined itself and
        // joined with this pair on both sides (the two cells of a side share a tile, so
        // k_spk_local left them under one label)
        const double pa = in[a - back], pb = in[b - back];
        if (!dm_is_hole(pa) && !dm_is_hole(pb) && spk_joined(va, pa, max_diff) && spk_joined(vb, pb, max_diff) &&
            spk_joined(pa, pb, max_diff))
            return;
    }
    spk_gunion(L, a, b);
}

// `acc` cells of root r into the tile's table (r < 0: nothing).  At most T T keys in 2 T T
// slots, and a key is never taken out: the probe meets a free slot or the key itself.
__device__ __forceinline__ void spk_insert(int *key, uint32_t *cnt, int r, uint32_t acc)
{
    if (r < 0) return;
    uint32_t h = ((uint32_t)r * 2654435761u) >> (32 - SPK_SLOT_BITS);
    for (;;) {
        const int old = atomicCAS(&key[h], -1, r);
        if (old == -1 || old == r) break;
        h = (h + 1) & (SPK_SLOTS - 1);
    }
    atomicAdd(&cnt[h], acc);
}

// Every cell's label becomes its root; S[root] receives the segment's size.  grid as
// k_spk_local.  LDS: key [SPK_SLOTS] roots (-1: free), cnt [SPK_SLOTS] cells of this tile.
__global__ __launch_bounds__(SPK_THREADS) void k_spk_count(int H, int W, int ts, int32_t *L, uint32_t *S)
{
    __shared__ int key[SPK_SLOTS];
    __shared__ uint32_t cnt[SPK_SLOTS];
    const int T = 1 << ts, cells = T * T;
    const size_t mbase = (size_t)blockIdx.z * H * W;
    L += mbase;
    S += mbase;
    const int y0 = blockIdx.y << ts, x0 = blockIdx.x << ts;
    for (int s = threadIdx.x; s < SPK_SLOTS; s += SPK_THREADS) {
        key[s] = -1;
        cnt[s] = 0;
    }
    __syncthreads();
    // a thread's cells lie in one column, SPK_THREADS / T rows apart: runs of one root are
    // counted in a register and inserted once
    int prev = -1;
    uint32_t acc = 0;
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        int r = -1;      // a hole, or a cell outside the map
        const int y = y0 + (l >> ts), x = x0 + (l & (T - 1));
        if (y < H && x < W) {
            const int g = y * W + x;
            const int p = L[g];
            if (p >= 0) {
                r = p;
                for (;;) {      // parents decrease down to the root; no union runs in this launch
                    const int q = L[r];
                    if (q == r) break;
                    r = q;
                }
                if (r != p) L[g] = r;
            }
        }
        if (r == prev) {
            ++acc;
            continue;
        }
        spk_insert(key, cnt, prev, acc);
        prev = r;
        acc = 1;
    }
    spk_insert(key, cnt, prev, acc);
    __syncthreads();
    for (int s = threadIdx.x; s < SPK_SLOTS; s += SPK_THREADS)
        if (key[s] >= 0) atomicAdd(&S[key[s]], cnt[s]);      // one add per (tile, root)
}

// The outputs of one cell from its input x, its label and its segment's size.
__device__ __forceinline__ void spk_write(size_t g, unsigned long long bits, int label, uint32_t size, int max_size,
                                          unsigned long long *out, uint8_t *removed, uint32_t *osize, int32_t *olabel)
{
    const bool rm = label >= 0 && size <= (uint32_t)max_size;
    out[g] = rm ? 0x7ff8000000000000ULL : bits;
    if (removed) removed[g] = rm ? 1 : 0;
    if (osize) osize[g] = label >= 0 ? size : 0;
    if (olabel) olabel[g] = label;
}

// grid (ceil(H W / SPK_THREADS), M)
__global__ __launch_bounds__(SPK_THREADS) void k_spk_apply(const unsigned long long *in, int cells, int max_size,
                                                           const int32_t *L, const uint32_t *S,
                                                           unsigned long long *out, uint8_t *removed,
                                                           uint32_t *osize, int32_t *olabel)
{
    const unsigned c = blockIdx.x * (unsigned)SPK_THREADS + threadIdx.x;
    if (c >= (unsigned)cells) return;
    const size_t mbase = (size_t)blockIdx.y * cells;
    const size_t g = mbase + c;
    const int label = L[g];
    const uint32_t size = label >= 0 ? S[mbase + label] : 0;
    spk_write(g, in[g], label, size, max_size, out, removed, osize, olabel);
}

// A map of at most T x T cells per workgroup, grid M: label, count and apply in LDS.
__global__ __launch_bounds__(SPK_THREADS) void k_spk_one(const double *in, int H, int W, int ts, int max_size,
                                                         double max_diff, unsigned long long *out, uint8_t *removed,
                                                         uint32_t *osize, int32_t *olabel)
{
    extern __shared__ double spk_lds[];
    const int T = 1 << ts, cells = T * T;
    double *V = spk_lds;
    int *P = (int *)(V + cells);
    uint32_t *C = (uint32_t *)(P + cells);
    const size_t mbase = (size_t)blockIdx.x * H * W;
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) C[l] = 0;
    spk_tile_label(in + mbase, H, W, 0, 0, ts, max_diff, V, P);      // (its barriers cover C)
    int prev = -1;
    uint32_t acc = 0;
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        const int r = P[l];
        if (r == prev) {
            ++acc;
            continue;
        }
        if (prev >= 0) atomicAdd(&C[prev], acc);
        prev = r;
        acc = 1;
    }
    if (prev >= 0) atomicAdd(&C[prev], acc);
    __syncthreads();
    for (int l = threadIdx.x; l < cells; l += SPK_THREADS) {
        const int y = l >> ts, x = l & (T - 1);
        if (y >= H || x >= W) continue;
        const int r = P[l];
        spk_write(mbase + (size_t)y * W + x, (unsigned long long)__double_as_longlong(V[l]),
                  r < 0 ? -1 : (r >> ts) * W + (r & (T - 1)), r < 0 ? 0 : C[r], max_size, out, removed, osize, olabel);
    }
}

// ---- host side ------------------------------------------------------------------------------
struct SpkPlan {
    size_t label, size;      // byte offsets into the workspace
    size_t bytes;
};

// false for a shape the entry does not take
static bool spk_plan(int32_t M, int32_t H, int32_t W, SpkPlan *p)
{
    if (!dm_maps_plan(M, H, W, SPK_TMAX * 65535)) return false;      // labels are int32; grid y / z
    const size_t c = (size_t)M * H * W;
    p->label = 0;
    p->size = (c * sizeof(int32_t) + 15) & ~(size_t)15;
    p->bytes = p->size + ((c * sizeof(uint32_t) + 15) & ~(size_t)15);
    return true;
}

// log2 of the tile side: 6, or that of DM_SPECKLE_TILE (16, 32 or 64) for measurements and
// tests (the result does not depend on it).  A side too small for the grid limits of the
// shape is not taken.
static int spk_tile_shift(int32_t H, int32_t W)
{
    int ts = dm_tile_env("DM_SPECKLE_TILE");
    if (!ts) ts = 6;
    if ((((long long)H + (1 << ts) - 1) >> ts) > 65535 || (((long long)W + (1 << ts) - 1) >> ts) > 65535) ts = 6;
    return ts;
}

extern "C" {

size_t dm_speckle_bytes(int32_t M, int32_t H, int32_t W)
{
    SpkPlan p;
    return spk_plan(M, H, W, &p) ? p.bytes : 0;
}

int dm_filter_speckles(const double *d_in, int32_t M, int32_t H, int32_t W, int32_t max_size, double max_diff,
                       double *d_out, uint8_t *d_removed, uint32_t *d_size, int32_t *d_label, void *d_work,
                       void *stream)
{
    if (!d_in || !d_out || !d_work) return dm_fail(DM_ERR_ARG, "null input / output / workspace pointer");
    if (M < 1 || H < 1 || W < 1) return dm_fail(DM_ERR_ARG, "bad speckle shape M=%d H=%d W=%d", M, H, W);
    if (max_size < 0) return dm_fail(DM_ERR_ARG, "max_size must be >= 0 (got %d)", max_size);
    if (!(max_diff >= 0.0)) return dm_fail(DM_ERR_ARG, "max_diff must be >= 0 (got %g)", max_diff);
    SpkPlan p;
    if (!spk_plan(M, H, W, &p))
        return dm_fail(DM_ERR_UNSUPPORTED,
                     "speckle filter of %d maps of %d x %d cells (at most 65535 maps of 2^31 - 1 cells)", M, H, W);
    hipStream_t st = (hipStream_t)stream;
    static bool attr_set = false; // idempotent attributes, benign race
    if (!attr_set) {
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_spk_one, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)SPK_ONE_LDS));
        DM_HIP_TRY(hipFuncSetAttribute((const void *)k_spk_local, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)SPK_LOCAL_LDS));
        attr_set = true;
    }
    const int ts = spk_tile_shift(H, W);
    const int T = 1 << ts;
    const size_t tc = (size_t)T * T;
    if (H <= T && W <= T) {      // the whole map in one tile: one launch, no workspace
        k_spk_one<<<M, SPK_THREADS, tc * (sizeof(double) + sizeof(int) + sizeof(uint32_t)), st>>>(
            d_in, H, W, ts, max_size, max_diff, (unsigned long long *)d_out, d_removed, d_size, d_label);
        DM_HIP_TRY(hipGetLastError());
        return DM_OK;
    }
    int32_t *L = (int32_t *)((char *)d_work + p.label);
    uint32_t *S = (uint32_t *)((char *)d_work + p.size);
    const dim3 grid((W + T - 1) >> ts, (H + T - 1) >> ts, M);
    k_spk_local<<<grid, SPK_THREADS, tc * (sizeof(double) + sizeof(int)), st>>>(d_in, H, W, ts, max_diff, L, S);
    DM_HIP_TRY(hipGetLastError());
    k_spk_border<<<grid, 2 * SPK_TMAX, 0, st>>>(d_in, H, W, ts, max_diff, L);
    DM_HIP_TRY(hipGetLastError());
    k_spk_count<<<grid, SPK_THREADS, 0, st>>>(H, W, ts, L, S);
    DM_HIP_TRY(hipGetLastError());
    const int cells = H * W;
    const dim3 agrid((unsigned)(((long long)cells + SPK_THREADS - 1) / SPK_THREADS), M);
    k_spk_apply<<<agrid, SPK_THREADS, 0, st>>>((const unsigned long long *)d_in, cells, max_size, L, S,
                                               (unsigned long long *)d_out, d_removed, d_size, d_label);
    DM_HIP_TRY(hipGetLastError());
    return DM_OK;
}

} // extern "C"
