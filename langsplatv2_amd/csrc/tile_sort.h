// tile_sort.h — the tile sort's size classes, shared by the sort (tile_sort.hip)
// and the binning pass that builds the class lists (binning.hip k_bin_table).
#pragma once
#include "lsr_internal.h"

#define LSR_SORT_WAVE_MAX 1024   // largest tile sorted by one wave in registers: 16 keys per lane

namespace lsr {

// Sort size classes: 0 one-wave sort (n <= LSR_SORT_WAVE_MAX), 1..3 block
// merge sorts with KPL = 8, 16, 32 (n <= 256*KPL), 4 chunked LDS/global
// (n > 8192).  Empty tiles are in no class.
__host__ __device__ __forceinline__ int tile_class(int n)
{
    if (n <= 0) return -1;
    if (n <= LSR_SORT_WAVE_MAX) return 0;
    if (n <= 2048) return 1;
    if (n <= 4096) return 2;
    if (n <= 8192) return 3;
    return 4;
}

// Wave-aggregated append of tile t (lanes with active) to its class list.
// Every lane of the wave must call it.  One atomic instruction for the whole
// wave: lane k adds the wave's class-k count to cls_cnt[k] (the classes'
// adds are independent, so they share one round trip instead of one each).
__device__ __forceinline__ void tile_class_append(bool active, int t, int n, int T, uint32_t* __restrict__ cls_cnt,
                                                  uint32_t* __restrict__ cls_list)
{
    const int c = active ? tile_class(n) : -1;
    const int lane = threadIdx.x & 63;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint64_t m[SORT_NCLS];
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < SORT_NCLS; k++) {
        m[k] = __ballot(c == k);
        cnt = lane == k ? (uint32_t)__popcll(m[k]) : cnt;
    }
    uint32_t base = 0;
    if (cnt) base = atomicAdd(&cls_cnt[lane], cnt);
    uint64_t mine = 0;
#pragma unroll
    for (int k = 0; k < SORT_NCLS; k++) mine = c == k ? m[k] : mine;
    const uint32_t b = __shfl(base, c < 0 ? 0 : c, 64);
    if (c >= 0) cls_list[(size_t)c * T + b + __popcll(mine & below)] = (uint32_t)t;
}

}  // namespace lsr
