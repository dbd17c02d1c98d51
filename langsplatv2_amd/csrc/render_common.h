// render_common.h — what the render translation units share.  The render is
// per-pixel alpha blending over the per-tile depth-ordered Gaussian lists
//  and its reverse replay (A.4), one kernel family per
// file: render_fwd.hip (dense forward), render_quick.hip (sparse "quick"
// forward), render_bwd.hip (dispatch order + factorised backward),
// render_det.hip (the deterministic backward's bounds / shifts / finish).
//
// Work decomposition (both directions): one 64-thread workgroup = ONE wave
// per 8x8 pixel block, four blocks per 16x16 tile, 4T workgroups.  Waves of
// a tile never synchronise with each other (no __syncthreads anywhere), so a
// wave whose pixels saturate retires immediately instead of idling at a block
// barrier; the four blocks of a tile are placed consecutively inside one
// XCD's dispatch range (WaveTile / xcd_remap) so they share that XCD's L2.
//
// Per chunk of 64 tile instances a wave loads the ids (prefetched one chunk
// ahead), the 32-B splat records and feature rows, tests each against its
// 8x8 block with the per-Gaussian cut ellipse (block_overlap), and compacts
// the survivors in order with __ballot + mbcnt into its private LDS stage.
// The per-pixel blend recurrence (alpha, transmittance, early termination)
// is serial and stays on the VALU, two candidates per step (two independent
// exp chains in flight).  For D > 8 the language channels accumulate on the
// matrix cores (the ML form of k_render_fwd: per 4 candidates the 4 x 64
// weights aT are transposed in registers into the B operand of
// v_mfma_f32_16x16x4_f32, bitwise the sequential fmaf chain); the quick path
// adds its sparse codes into register-resident accumulators.
//
// Backward (k_render_bwd_mf): same mapping, instances replayed back to front
// from the wave's largest n_contrib in groups of 16 candidates: alpha/G per
// candidate (phase 1), the serial transmittance recurrence (phase 2), then
// every per-Gaussian pixel sum as a contraction — language on exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32), colour and the six geometry moments on the VALU —
// added with line-coalesced buffer atomics (see the comment at the kernel).
#pragma once
#include "lsr_internal.h"

#include <type_traits>
#include <utility>

namespace lsr {

// ----------------------------------------------------------- reductions --
__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ float wave_max_f(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// ------------------------------------------------------ work mapping ------
// Lane -> pixel mapping: wave w of the tile owns the 8x8 block
// (w & 1, w >> 1); lane l owns pixel (l & 7, l >> 3) of it.
struct PixMap {
    int bx, by, px, py;
    __device__ PixMap(const Cam& c, int tile, int t)
    {
        const int tx = tile % c.gx, ty = tile / c.gx;
        const int w = t >> 6, l = t & 63;
        bx = tx * LSR_TILE + (w & 1) * 8;
        by = ty * LSR_TILE + (w >> 1) * 8;
        px = bx + (l & 7);
        py = by + (l >> 3);
    }
};

// Work-item mapping for the wave-independent render kernels: one 64-thread
// workgroup (one wave) per 8x8 block; the four blocks of a tile get
// consecutive indices inside one XCD's range (xcd_remap), so they share an L2.
//
// Inside its range an XCD walks the tiles in band order (band_tile): bands of
// LSR_BAND tile rows, column by column inside a band.  A Gaussian's tiles are
// then visited close together in time, so the lines its blocks read (records,
// feature rows) and the backward's gradient lines its atomics update are
// still in that XCD's L2 (row-major order revisits them a whole tile row
// later, after ~6 MB of other lines have passed through the 4 MB L2).
#ifndef LSR_BAND
#define LSR_BAND 4          // tile rows per band; 0 = row-major tile order (cfg3 sum 1.487 -> 1.479 ms, cfg5 fwd 1.93 -> 1.88)
#endif
__device__ __forceinline__ int band_tile(int t, int gx, int gy)
{
    if (LSR_BAND <= 0) return t;
    const int per = gx * LSR_BAND;
    const int b = t / per, r = t - b * per;
    const int rows = min(LSR_BAND, gy - b * LSR_BAND);
    const int col = r / rows;
    return (b * LSR_BAND + (r - col * rows)) * gx + col;
}
struct WaveTile {
    int tile, sub;
    // with an order: the block's tile range and list count from the same entry
    // (one load before the wave can start its list DMA and fragment loads)
    uint32_t rs = 0u, re = 0u, lc = 0u;
    bool ent = false;
    // order (the backward's RenderArgs::border): dispatch slot -> block 4 tile + sub
    __device__ WaveTile(const RenderArgs& a, const uint4* order = nullptr)
    {
        const int o = xcd_remap(blockIdx.x, gridDim.x);
        if (order) {
            const uint4 e = order[o];
            tile = (int)(e.x >> 2);
            sub = (int)(e.x & 3u);
            rs = e.y;
            re = e.z;
            lc = e.w;
            ent = true;
        } else {
            tile = band_tile(o >> 2, a.cam.gx, a.cam.gy);
            sub = o & 3;
        }
    }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------ host dispatch -----
// The launchers pick a kernel instantiation from runtime values: each helper
// turns one value into a compile-time constant and calls a generic lambda with
// it; an `if constexpr` in the lambda keeps a combination from being compiled.

// The compiled dense language channel sets, ascending (lang_set_for rounds D up).
using LangSets = std::integer_sequence<int, 0, 4, 8, 16, 32, 64>;

template <int... NL>
constexpr int lang_set_ceil(std::integer_sequence<int, NL...>, int D)
{
    int r = -1;
    ((r = (r < 0 && D <= NL) ? NL : r), ...);
    return r;
}

// f(std::integral_constant<int, V>) for the V of the list that equals v and is
// at least MIN; false (f not called, nothing below MIN compiled) if there is none
template <int MIN = 0, int... V, class F>
bool with_int(std::integer_sequence<int, V...>, int v, F&& f)
{
    auto one = [&](auto c) {
        if constexpr (c.value >= MIN) {
            if (v == c.value) return f(c), true;
        }
        return false;
    };
    return (one(std::integral_constant<int, V>{}) || ...);
}
template <int MIN = 0, class F>
bool with_lang_set(int nl, F&& f)
{
    return with_int<MIN>(LangSets{}, nl, f);
}

// (with_bools, for runtime bools: lsr_internal.h)

}  // namespace lsr
