// render_det.hip — the deterministic backward (LSR_OPT_DETERMINISTIC) around
// the render: before it, the gradient bounds and per-Gaussian fixed-point
// exponents (k_det_bounds, k_det_reduce, k_det_shifts); after it, the 64-bit
// sums back to fp32 (k_det_finish).  The adds themselves are the DET form of
// k_render_bwd_mf (render_bwd.hip); the format is render_det.h.
#include "render_common.h"
#include "render_det.h"

#include <algorithm>

namespace lsr {

// ------------------------------------------ deterministic backward: bounds
// max |dL/dout| over the 3 + D upstream planes and max |feature| over the
// visible Gaussians' colours and the dense language input (order-independent);
// bit 0 of word 2 flags a non-finite value.  Blocks [0, nbd) read the three
// arrays as one float4 index space, 8 loads in flight per lane (a strided loop
// per array left a chain of dependent rounds); blocks below gridDim - nbd take
// one visible Gaussian's row per thread.
__device__ __forceinline__ void det_max4(float4 v, float& m, bool& bad)
{
    bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}

__global__ void __launch_bounds__(256) k_det_bounds(const float* __restrict__ dc, const float* __restrict__ dl,
                                                    uint32_t ncol, uint32_t nlang, int nbd,
                                                    const float* __restrict__ lang, uint32_t nfeat,
                                                    const float* __restrict__ rgb, const int32_t* __restrict__ radii,
                                                    int P, float* bounds)
{
    float md = 0.f, mf = 0.f;
    bool bad = false;
    // the colour blocks first (their dependent radius -> colour loads then
    // overlap the stream instead of trailing it)
    const int nbf = (int)gridDim.x - nbd;
    const int blk = (int)blockIdx.x - nbf;
    if (blk >= 0) {
        // float4 parts of the aligned arrays: [colour planes | language planes | language input]
        auto n4 = [](const float* p, uint32_t n) { return (p && ((uintptr_t)p & 15u) == 0) ? n / 4 : 0u; };
        const uint32_t N1 = n4(dc, ncol), N2 = N1 + n4(dl, nlang), N3 = N2 + n4(lang, nfeat);
        const float4* c4 = reinterpret_cast<const float4*>(dc);
        const float4* l4 = reinterpret_cast<const float4*>(dl);
        const float4* f4 = reinterpret_cast<const float4*>(lang);
        // block chunks of 4 x 256 consecutive float4 (a copy's access pattern)
        const uint32_t nch = (N3 + 1023) / 1024;
        for (uint32_t ch = (uint32_t)blk; ch < nch; ch += (uint32_t)nbd) {
            float4 v[4];
            uint32_t ec[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                // branch-free: past the end, lanes re-read the last element (a
                // real one, counted where it belongs)
                ec[k] = min(ch * 1024u + (uint32_t)k * 256u + threadIdx.x, N3 - 1);
                const float4* q = ec[k] < N1 ? c4 + ec[k] : (ec[k] < N2 ? l4 + (ec[k] - N1) : f4 + (ec[k] - N2));
                v[k] = *q;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool isd = ec[k] < N2;
                float m = isd ? md : mf;
                det_max4(v[k], m, bad);
                md = isd ? m : md;
                mf = isd ? mf : m;
            }
        }
        const uint32_t stride = (uint32_t)nbd * blockDim.x, b0 = (uint32_t)blk * blockDim.x + threadIdx.x;
        // the scalar rest: tails past the float4 parts, or a whole misaligned array
        auto rest = [&](const float* p, uint32_t n, float& m) {
            if (!p) return;
            for (uint32_t e = 4 * n4(p, n) + b0; e < n; e += stride) {
                const float x = p[e];
                bad |= !isfinite(x);
                m = fmaxf(m, fabsf(x));
            }
        };
        rest(dc, ncol, md);
        rest(dl, nlang, md);
        rest(lang, nfeat, mf);
    } else {
        // the colours of the visible Gaussians (a culled Gaussian's colour is never written)
        const int stride = nbf * (int)blockDim.x;
        for (int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x; i < P; i += stride) {
            if (radii[i] <= 0) continue;
            for (int c = 0; c < 3; c++) {
                const float v = rgb[3 * (size_t)i + c];
                bad |= !isfinite(v);
                mf = fmaxf(mf, fabsf(v));
            }
        }
    }
    // the block's partial to its own slot (same-address atomics serialise: one
    // per wave over ~6 K blocks cost 0.3 ms, one per block over 1.3 K 0.05 ms);
    // k_det_reduce folds the slots
    __shared__ float smd[4], smf[4];
    __shared__ uint32_t sbad[4];
    md = wave_max_f(md);
    mf = wave_max_f(mf);
    const bool wbad = wave_ballot(bad) != 0u;
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smd[w] = md;
        smf[w] = mf;
        sbad[w] = wbad ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* part = bounds + 64;
        part[blockIdx.x] = fmaxf(fmaxf(smd[0], smd[1]), fmaxf(smd[2], smd[3]));
        part[LSR_DET_BLOCKS + blockIdx.x] = fmaxf(fmaxf(smf[0], smf[1]), fmaxf(smf[2], smf[3]));
        reinterpret_cast<uint32_t*>(part)[2 * LSR_DET_BLOCKS + blockIdx.x] = sbad[0] | sbad[1] | sbad[2] | sbad[3];
    }
}

// per Gaussian, det_shift of the four column classes as signed bytes (the
// adds and the conversion read the same table, so their exponents agree by
// construction)
__global__ void __launch_bounds__(256) k_det_shifts(const int32_t* __restrict__ radii, const float* __restrict__ bounds,
                                                    int P, int D, const float* __restrict__ bg, float WH,
                                                    uint32_t* __restrict__ sh)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float Dm = bounds[0];
    const float Am = (2.f * (float)(3 + D) * bounds[1] + (fabsf(bg[0]) + fabsf(bg[1]) + fabsf(bg[2]))) * Dm;
    const int r = radii[i];
    uint32_t w = 0u;
#pragma unroll
    for (int cls = 0; cls < 4; cls++) w |= ((uint32_t)det_shift(cls, r, Dm, Am, WH) & 0xffu) << (8 * cls);
    sh[i] = w;
}

// one block: the nb partials -> bounds[0..2]
__global__ void __launch_bounds__(1024) k_det_reduce(float* bounds, int nb)
{
    const float* part = bounds + 64;
    float md = 0.f, mf = 0.f;
    uint32_t bad = 0u;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        md = fmaxf(md, part[i]);
        mf = fmaxf(mf, part[LSR_DET_BLOCKS + i]);
        bad |= reinterpret_cast<const uint32_t*>(part)[2 * LSR_DET_BLOCKS + i];
    }
    __shared__ float smd[16], smf[16];
    __shared__ uint32_t sbad[16];
    md = wave_max_f(md);
    mf = wave_max_f(mf);
    const bool wbad = wave_ballot(bad != 0u) != 0u;
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smd[w] = md;
        smf[w] = mf;
        sbad[w] = wbad ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (int)(blockDim.x + 63) / 64;
        for (int k = 1; k < nw; k++) {
            md = fmaxf(md, smd[k]);
            mf = fmaxf(mf, smf[k]);
            sbad[0] |= sbad[k];
        }
        bounds[0] = md;
        bounds[1] = mf;
        reinterpret_cast<uint32_t*>(bounds)[2] = sbad[0];
    }
}

hipError_t launch_det_bounds(const RenderBwdArgs& b, float* bounds, hipStream_t st)
{
    const size_t HW = (size_t)b.f.cam.W * b.f.cam.H;
    const int D = b.f.D;
    if (D > 0 && (!b.dout_lang || !b.f.lang)) return hipErrorInvalidValue;
    if (!b.det_sh || !b.radii) return hipErrorInvalidValue;
    const size_t nf = (size_t)b.f.P * (size_t)(D > 0 ? D : 0);
    if (3 * HW >= (1ull << 32) || (size_t)D * HW >= (1ull << 32) || nf >= (1ull << 32)) return hipErrorInvalidValue;
    // one 16-KB chunk per scan block; one Gaussian per colour thread
    const size_t n4 = (3 * HW + (size_t)D * HW + nf) / 4;
    const int nbd = (int)std::max<size_t>(1, std::min<size_t>((n4 + 1023) / 1024, LSR_DET_BLOCKS - LSR_DET_BLOCKS / 4));
    const int nbf = std::max(1, std::min((b.f.P + 255) / 256, LSR_DET_BLOCKS / 4));
    k_det_bounds<<<nbd + nbf, 256, 0, st>>>(b.dout_color, D > 0 ? b.dout_lang : nullptr, (uint32_t)(3 * HW),
                                            (uint32_t)((size_t)D * HW), nbd, D > 0 ? b.f.lang : nullptr,
                                            (uint32_t)nf, b.f.rgb, b.radii, b.f.P, bounds);
    k_det_reduce<<<1, 1024, 0, st>>>(bounds, nbd + nbf);
    if (b.f.P > 0)
        k_det_shifts<<<(b.f.P + 255) / 256, 256, 0, st>>>(b.radii, bounds, b.f.P, D, b.f.cam.bg,
                                                          (float)std::max(b.f.cam.W, b.f.cam.H), b.det_sh);
    return hipGetLastError();
}

// ---------------------------------------- deterministic backward: to fp32
// mode 0: rows (P, VP) generic layout ([0..8] geometry + colour, [12, 12 + D)
// language) -> gout; mode 1 (lang_direct): rows (P, 16) -> gout, lang (P, D)
// -> lout; mode 2 (language only): rows (P, D) -> lout.  Every element of the
// outputs is written (unused row slots 0).  One thread per (Gaussian, 4
// columns), 32-bit index arithmetic.
__device__ __forceinline__ float det_value(long long acc, int s)
{
    return acc != 0 ? (float)ldexp((double)acc, -s) : 0.f;
}

__global__ void __launch_bounds__(256) k_det_finish(const long long* __restrict__ rows,
                                                    const long long* __restrict__ lang,
                                                    const uint32_t* __restrict__ shifts,
                                                    const float* __restrict__ bounds, int P, int VP, int D, int mode,
                                                    float* __restrict__ gout, float* __restrict__ lout)
{
    // column quads per Gaussian: the row part, then (mode 1) the language part
    const int wr = mode == 2 ? D : VP;
    const int qr = (wr + 3) / 4;
    const int ql = mode == 1 ? (D + 3) / 4 : 0;
    const int qn = qr + ql;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = t / (uint32_t)qn;
    if (i >= (uint32_t)P) return;
    const int q = (int)(t - i * (uint32_t)qn);
    const bool bad = (__float_as_uint(bounds[2]) & 1u) != 0u;
    const uint32_t sw = shifts[i];   // the exponents the adds used
    const bool in_rows = q < qr;
    const int c0 = 4 * (in_rows ? q : q - qr);
    const int w = in_rows ? wr : D;
    const long long* src = (in_rows ? rows : lang) + (size_t)i * w;
    float* dst = (in_rows && mode != 2 ? gout : lout) + (size_t)i * w;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int col = c0 + k;
        int cls = 0;
        bool used = col < w;
        if (in_rows && mode != 2) {
            used = used && (col < 9 || (mode == 0 && col >= LSR_GROW_LANG && col < LSR_GROW_LANG + D));
            cls = det_class_of(col);
        }
        const long long acc = used ? src[col] : 0;
        v[k] = bad ? __builtin_nanf("") : det_value(acc, (int)(int8_t)(sw >> (8 * cls)));
    }
    if (c0 + 4 <= w && ((uintptr_t)(dst + c0) & 15u) == 0) {
        *reinterpret_cast<float4*>(dst + c0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c0 + k < w) dst[c0 + k] = v[k];
    }
}

hipError_t launch_det_finish(const RenderBwdArgs& b, bool lang_only, float* grad_out, float* lang_out, hipStream_t st)
{
    const int P = b.f.P, D = b.f.D;
    const int mode = lang_only ? 2 : (b.det_lang ? 1 : 0);
    if (!b.det_rows || !b.det_bounds || !b.det_sh || (mode == 0 && !grad_out) || (mode != 0 && !lang_out) ||
        (mode == 1 && !grad_out))
        return hipErrorInvalidValue;
    const int wr = mode == 2 ? D : b.VP;
    const int qn = (wr + 3) / 4 + (mode == 1 ? (D + 3) / 4 : 0);
    const size_t n = (size_t)P * (size_t)qn;
    if (n == 0) return hipSuccess;
    if (n >= (1ull << 32)) return hipErrorInvalidValue;
    k_det_finish<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(b.det_rows, b.det_lang, b.det_sh, b.det_bounds, P, b.VP,
                                                              D, mode, grad_out, lang_out);
    return hipGetLastError();
}
}  // namespace lsr
