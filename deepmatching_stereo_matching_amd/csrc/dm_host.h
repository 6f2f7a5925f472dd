// dm_host.h -- what every .hip file of the library shares outside its kernels: error reporting
// over the one thread-local message of dm_kernels.hip, the hole test and the quiet NaN of the
// d_map stages, the shape limits of their entries and the DM_*_TILE override.
#ifndef DM_HOST_H
#define DM_HOST_H

#include <hip/hip_runtime.h>

#include <float.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/dmstereo.h"

// defined in dm_kernels.hip (not exported): formats into the calling thread's message, returns code
__attribute__((visibility("hidden"))) int dm_vfail(int code, const char *fmt, va_list ap);

__attribute__((unused)) static int dm_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    const int r = dm_vfail(code, fmt, ap);
    va_end(ap);
    return r;
}

#define DM_HIP_TRY(x)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) return dm_fail(DM_ERR_HIP, "HIP error: %s (%d)", hipGetErrorString(e_), (int)e_); \
    } while (0)

// a hole of a map: the range test on the double itself, NaN and +-inf fail it
__host__ __device__ __forceinline__ bool dm_is_hole(double x) { return !(x >= -DBL_MAX && x <= DBL_MAX); }

// the quiet NaN a stage writes into a hole (called from device code only)
__host__ __device__ __forceinline__ double dm_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the shapes an entry over M maps of H x W cells takes: at most 65535 maps (grid y / z) of 2^31 - 1
// cells (int32 cell indices), no side above side_max (the tile side times 65535 tiles)
__attribute__((unused)) static bool dm_maps_plan(int32_t M, int32_t H, int32_t W, int32_t side_max)
{
    if (M < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return false;
    return M <= 65535 && H <= side_max && W <= side_max;
}

// log2 of the tile side that the environment variable `name` forces (16 or 32, for measurements
// and tests: no result depends on the tile), 0 when it forces none
__attribute__((unused)) static int dm_tile_env(const char *name)
{
    const char *e = getenv(name);
    const int v = e && *e ? atoi(e) : 0;
    return v == 16 ? 4 : v == 32 ? 5 : 0;
}

#endif
