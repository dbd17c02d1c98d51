// quick_common.h — what the consumers of the quick language map share:
// quick_decode.hip (codebook decode), quick_query.hip
// (fused text-query relevancy) and quick_heat.hip (the viewer's maps).  All
// are split-f16 MFMA products on the same A fragments: every f32 operand x is
// split into x_hi = f16(x), x_lo = f16(x - x_hi) (22 significant bits together) and
//   F = W_hi C_hi + W_hi C_lo + W_lo C_hi
// runs on v_mfma_f32_16x16x32_f16 with f32 accumulation: the products are
// exact in f32, the dropped W_lo C_lo term is <= 2^-22 |W||C|, i.e. within a
// few f32 ulps of the exact-f32 product.  The B operand (codebook, norm factor
// or query projection) is scaled per level by a power of two into [0.5, 1)
// before the split (f16 range; exact) and the scale is applied to the results.
//
// Orientation: A = W^T (rows = 16 pixels along x, K = codes), B = (K = codes,
// cols = 16 output columns), so a lane's result is 4 CONSECUTIVE pixels of one
// output column.  Here: the tile front end of the level-resident kernels (the
// weight-tile load for both map layouts, the per-pixel power-of-two scaling,
// the f16 split), the split product and the 16-lane reductions.
#pragma once
#include "lsr_internal.h"

namespace lsr {

typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

#ifndef LSR_DEC2_WAVES
#define LSR_DEC2_WAVES 8     // waves per level-resident workgroup (one workgroup per CU: LDS)
#endif
#define LSR_DEC2_MAXDB 32    // Df <= 512: fragments + norm factor fit in 144 KB of LDS

// 16-lane sum (every lane of each 16-lane row gets its row's total)
__device__ __forceinline__ float row16_sum(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));   // quad [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));  // row_mirror
    return v;
}

// 16-lane max (every lane of each 16-lane row gets its row's maximum)
__device__ __forceinline__ float row16_max(float v)
{
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));
    return v;
}

// F tile of pixel row pb for one 16-column block: the split product, small terms first
#define LSR_DEC_MFMA6(acc, pb)                                                                  \
    do {                                                                                        \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wl[pb][0], c0h, acc, 0, 0, 0);             \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wh[pb][0], c0l, acc, 0, 0, 0);             \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wl[pb][1], c1h, acc, 0, 0, 0);             \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wh[pb][1], c1l, acc, 0, 0, 0);             \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wh[pb][0], c0h, acc, 0, 0, 0);             \
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(Wh[pb][1], c1h, acc, 0, 0, 0);             \
    } while (0)

// Exchange a register bit with lane bit log2(D) (D = 4 or 8) between X (bit 0)
// and Y (bit 1): X's lanes with the lane bit set take Y's lanes D below, Y's
// lanes with it clear take X's lanes D above (DPP row shifts within 16-lane
// rows; bank masks select the 4-lane banks written).
template <int D>
__device__ __forceinline__ void dec_swap_lanebit(f32x4q& X, f32x4q& Y)
{
    static_assert(D == 4 || D == 8, "lane bit 2 or 3");
    constexpr int SHR = 0x110 + D, SHL = 0x100 + D;
    constexpr int HI = D == 4 ? 0xA : 0xC, LO = D == 4 ? 0x5 : 0x3;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int x = __float_as_int(X[r]), y = __float_as_int(Y[r]);
        X[r] = __int_as_float(__builtin_amdgcn_update_dpp(x, y, SHR, 0xF, HI, false));
        Y[r] = __int_as_float(__builtin_amdgcn_update_dpp(y, x, SHL, 0xF, LO, false));
    }
}

// The tile front end of the level-resident kernels (k_quick_decode_l, k_quick_query).
// dec_load_tile: raw weights of 64-pixel tile tt of level l (a tile past the last reads
// tile 0 and gives zeros): lane (li, lg) holds raw[pb][s][j] = W[64 l + 32 s + 8 lg + j][x = bx + 16 pb + li].
// PB: the tile's 16-pixel blocks (the level-resident kernels' 4; k_quick_heat's tiles are narrower), nbx
// the 16 PB-pixel tiles of an image row.
// HWC: the weight map is pixel-major (H, W, lk) (LSR_LAYOUT_HWC): a lane's 8 codes
// of one pixel are 32 contiguous bytes, two 16-B loads instead of eight 4-B ones
// from eight channel planes.
template <bool HWC, int PB = 4>
__device__ __forceinline__ void dec_load_tile(float (&raw)[PB][2][8], const float* __restrict__ wmap, int tt, int ntile,
                                              int nbx, int W, size_t HW, int l, int lk, int li, int lg)
{
    const bool ok = tt < ntile;
    const int tq = ok ? tt : 0;
    const int bx = (tq % nbx) * (16 * PB), y = tq / nbx;
#pragma unroll
    for (int pb = 0; pb < PB; pb++) {
        const int xa = bx + 16 * pb + li;
        const size_t pa = (size_t)y * W + min(xa, W - 1);
        const bool in = ok && xa < W;
        if constexpr (HWC) {
            const float4* wp = reinterpret_cast<const float4*>(wmap + pa * lk + l * 64 + 8 * lg);
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
                const float4 v0 = wp[8 * s2], v1 = wp[8 * s2 + 1];
                raw[pb][s2][0] = in ? v0.x : 0.f;
                raw[pb][s2][1] = in ? v0.y : 0.f;
                raw[pb][s2][2] = in ? v0.z : 0.f;
                raw[pb][s2][3] = in ? v0.w : 0.f;
                raw[pb][s2][4] = in ? v1.x : 0.f;
                raw[pb][s2][5] = in ? v1.y : 0.f;
                raw[pb][s2][6] = in ? v1.z : 0.f;
                raw[pb][s2][7] = in ? v1.w : 0.f;
            }
        } else {
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float v = wmap[(size_t)(l * 64 + 32 * s2 + 8 * lg + j) * HW + pa];
                    raw[pb][s2][j] = in ? v : 0.f;
                }
        }
    }
}

// Per-pixel power-of-two scaling of a tile's weights, then the f16 split: the
// pixel's largest |w| goes to [0.5, 1), so a nearly transparent pixel's small
// weights keep all 22 bits of hi + lo instead of falling into f16's subnormal
// range (exact: the caller undoes the scale, and the L2 norm is scale-
// invariant).  Lane (li, lg) holds pixel (pb, li); psc[pb] = 2^e of that
// pixel: w = psc * w_scaled.
// k_quick_query and k_quick_heat call this; k_quick_decode_l keeps the same statements written
// out in its tile loop, and a fix here must be made there too.  Calling it
// from the decode changes the compiler's code for all eight instantiations
// (the split comes out as packed v_pk_add_f32 / SDWA converts, fewer
// instructions, bit-equal results) and that code measured slower on an
// MI355X, alternating with the written-out form in one process: 1.332 vs
// 1.323 ms at 1280x800 and 3.021 vs 3.006 ms at 1920x1080 (3 x 64 x 512,
// normalised), with two builds of the written-out form 0.001 ms apart; the
// prefetch moved below the output-scale shuffles gave 1.328 / 3.023 ms, and
// helpers without __restrict__ or split in two compile to the same code
// (profiles/quick_split_ab_decode.txt).  dec_load_tile is shared by both:
// through a lambda the decode's code is instruction for instruction the same.
template <int PB>
__device__ __forceinline__ void dec_scale_split(float (&raw)[PB][2][8], float (&psc)[PB], h8 (&Wh)[PB][2],
                                                h8 (&Wl)[PB][2])
{
#pragma unroll
    for (int pb = 0; pb < PB; pb++) {
        float m = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
            for (int j = 0; j < 8; j++) m = fmaxf(m, fabsf(raw[pb][s2][j]));
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        int e = 0;
        if (m > 0.f && m < 3.0e38f) (void)frexpf(m, &e);
        // both factors stay finite normals: a subnormal m (e down to -148)
        // or m >= 2^127 would otherwise make inv or psc infinite
        e = min(max(e, -126), 126);
        psc[pb] = ldexpf(1.f, e);
        const float inv = ldexpf(1.f, -e);
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
            for (int j = 0; j < 8; j++) raw[pb][s2][j] *= inv;
    }
#pragma unroll
    for (int pb = 0; pb < PB; pb++)
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float v = raw[pb][s2][j];
                const _Float16 h = (_Float16)v;
                Wh[pb][s2][j] = h;
                Wl[pb][s2][j] = (_Float16)(v - (float)h);
            }
}

// the level-resident kernels run one workgroup per CU
inline int cu_count()
{
    static int ncu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    return ncu;
}

}  // namespace lsr
