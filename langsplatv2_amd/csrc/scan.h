// scan.h — wave and block scans shared by the uint32 scan (scan.hip) and the
// binning kernels (binning.hip).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace lsr {

// Inclusive scan over the wave's 64 lanes (shuffles; every lane must call it).
template <class T>
__device__ __forceinline__ T wave_incl_scan(T x)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// Block-wide exclusive scan over NB threads (sh: NB / 64 entries).
template <int NB>
__device__ __forceinline__ uint64_t block_excl_scan_u64_n(uint64_t v, uint64_t* sh, uint64_t& total)
{
    // the waves' inclusive scans, then across the waves through LDS
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t x = wave_incl_scan(v);
    if (lane == 63) sh[w] = x;
    __syncthreads();
    uint64_t wofs = 0, tot = 0;
    for (int k = 0; k < NB / 64; k++) {
        if (k < w) wofs += sh[k];
        tot += sh[k];
    }
    __syncthreads();
    total = tot;
    return wofs + x - v;
}

}  // namespace lsr
