// render_det.h — the deterministic backward's fixed-point format
// (LSR_OPT_DETERMINISTIC), shared by the backward kernel that adds in it
// (render_bwd.hip) and the kernels that choose its exponents and convert the
// sums back (render_det.hip).
#pragma once
#include "lsr_internal.h"

namespace lsr {

// Every per-Gaussian gradient is a sum over the 8x8 blocks the Gaussian is
// staged in of a per-block partial (the block's 64 pixels summed in a fixed
// order by its wave); only the order in which the blocks' atomics land varies.
// DET adds the partials as 64-bit fixed-point integers instead (associative:
// the same bits in any order).  The exponent of (Gaussian i, column class) is
// chosen from an a-priori bound of the partials (64 pixels x the per-pixel
// bound) and of how many blocks can contribute (the radius rect, nb =
// (r/4 + 2)^2 blocks), so the sum cannot overflow:
//   class 0 colour / language  aT |dL/dout|                        <= Dm
//   class 1 opacity            G |dL/dalpha|                       <= Am
//   class 2 mean2D (NDC)       0.5 W o G |conic d| |dL/dalpha|     <= 0.554 max(W,H) Am
//                              (|conic| <= 1/0.3 from the 0.3 dilation; sup sqrt(q) e^(-q/2) = e^(-1/2))
//   class 3 conic              0.5 o G |d|^2 |dL/dalpha|           <= 0.041 r^2 Am
//                              (G |d|^2 <= (2/e) lambda_max(cov2D) <= (2/e) (r/3)^2)
// with Dm = max |dL/dout| and Am = (2 C Fm + |bg|_1) Dm >= |dL/dalpha|
// (|dot|, |S| <= C Fm Dm for Fm = max |feature|, T <= 1, T_final / (1 - alpha) <= T).
// s = 61 - e(nb) - e(bound): every partial and every sum stays below 2^61 in
// fixed units (frexp exponent e: x < 2^e); one rounding per partial, at 2^-s.
__device__ __forceinline__ int det_class_of(int f)
{
    return f < 2 ? 2 : (f < 5 ? 3 : (f == 5 ? 1 : 0));
}

__device__ __forceinline__ int det_shift(int cls, int r, float Dm, float Am, float WH)
{
    const float rr = (float)max(r, 1);
    const float q = fmaf(0.25f, rr, 2.f);
    const float B = cls == 0 ? 64.f * Dm : (cls == 1 ? 64.f * Am : (cls == 2 ? 40.f * WH * Am : 3.f * rr * rr * Am));
    int en = 0, eb = 0;
    (void)frexpf(q * q, &en);
    (void)frexpf(fmaxf(B, 1e-30f), &eb);
    return min(max(61 - en - eb, -100), 100);
}

// adds v at 2^s; a value outside the bound (never, by the analysis above) or a
// non-finite one flags the call instead (the conversion then writes NaN)
__device__ __forceinline__ void det_add(long long* p, float v, int s, uint32_t* flag)
{
    const float x = ldexpf(v, s);
    if (!(fabsf(x) < 0x1p61f)) {
        atomicOr(flag, 1u);
        return;
    }
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__float2ll_rn(x));
}

}  // namespace lsr
