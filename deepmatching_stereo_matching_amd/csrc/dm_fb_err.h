// dm_fb_err.h -- the round-trip error of the forward-backward check (dm_fb.hip has the
// definition), shared by dm_fb.hip and dm_merge.hip.
#ifndef DM_FB_ERR_H
#define DM_FB_ERR_H

#include <hip/hip_runtime.h>

#include <math.h>

// round-trip error of cell l = i * w + j of one tile: f / b point at the tile's [3][h][w]
// forward / backward maps, P = h * w.  The index into b is formed only from values the
// floating-point range test has admitted: 0 <= qi < h, 0 <= qj < w.
__device__ __forceinline__ double fb_err(const double *f, const double *b, size_t P, int h, int w, int i, int j,
                                         size_t l)
{
    const double qi = floor(f[l] + 0.5), qj = floor(f[P + l] + 0.5);
    if (!(qi >= 0.0 && qi < (double)h && qj >= 0.0 && qj < (double)w)) return NAN;
    const size_t q = (size_t)(int)qi * w + (size_t)(int)qj;
    const double dr = b[q] - (double)i, dc = b[P + q] - (double)j;
    return sqrt(dr * dr + dc * dc);
}

#endif // DM_FB_ERR_H
