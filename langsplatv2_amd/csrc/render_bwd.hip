// render_bwd.hip — the render's reverse replay: the list-driven backward's
// dispatch order (k_bwd_order) and the factorised backward k_render_bwd_mf
// with its three launchers.  Work decomposition: render_common.h.
#include "render_common.h"
#include "render_det.h"

#ifndef LSR_BWD_SPLAT_PF
#define LSR_BWD_SPLAT_PF 1  // bwd: chunk records loaded one chunk ahead (ids two ahead), D <= 32
#endif
#ifndef LSR_BWD_LO_RREG
#define LSR_BWD_LO_RREG 1   // language-only bwd: atomics straight from the MFMA accumulators (no LDS row tile)
#endif
#ifndef LSR_BWD16_WAVES
#define LSR_BWD16_WAVES 4  // the headline D = 16 list-driven backward: waves per SIMD it is compiled for
#endif
#ifndef LSR_BWD_LD_STATIC
#define LSR_BWD_LD_STATIC 1  // direct-dL/dlang kernels: compile-time row strides, buffer atomics only (BA below)
#endif
#ifndef LSR_MF_WAVES
#define LSR_MF_WAVES 2      // MFMA render kernels: min waves per SIMD (caps VGPRs at 256)
#endif

namespace lsr {

// The list-driven backward's dispatch order.  A backward wave lasts about
// 5-8 us per 16-candidate group of its block list at cfg3, and with the
// blocks in band order the last waves to be dispatched are as heavy as any:
// the launch ended in a ~70 us drain with the machine less and less occupied
// (profiles/r06s_wtl.json: 86 % of the wave slots busy over the launch).
// XCD x's dispatch range (xcd_remap) now holds the blocks with the same
// range of NATURAL indices 4 tile + sub (a horizontal strip of tiles, so a
// tile's four blocks and most of a Gaussian's tiles still share that XCD's
// L2), in descending order of their list length in 16-candidate groups (the
// forward's lcount): the drain is made of the lightest blocks.  One
// workgroup per XCD range, an LDS counting sort, launched right after the
// forward render.  Speed only: every block is still processed exactly once.
// The sort costs L2 reuse (PMC fetch 344 -> 722 MB per launch) and still
// wins: a stable partition that keeps band order for all but the lightest
// quarter (moved to the end) fetched 462 MB and measured 0.457 ms against the
// sort's 0.450 (band order 0.470; profiles/r06za_ab_bwd_partition.txt).
// Keyed by the tile's instance count instead -- known before the render, so
// the sort could run on the colour stream during the binning -- it gained
// nothing: a block's list length does not follow its tile's count.
#define LSR_ORD_NB 64
#ifndef LSR_ORD_THREADS
#define LSR_ORD_THREADS 1024
#endif
#define LSR_ORD_KPT 16   // keys held per thread (ranges up to 16 x LSR_ORD_THREADS blocks in one pass)
__global__ void __launch_bounds__(LSR_ORD_THREADS) k_bwd_order(const uint32_t* __restrict__ lcount,
                                                    const uint32_t* __restrict__ tile_start, int n,
                                                    uint4* __restrict__ border)
{
    __shared__ uint32_t cnt[LSR_ORD_NB];
    const int q = n / 8, r = n % 8, x = blockIdx.x;
    const int lo = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    const int len = q + (x < r ? 1 : 0);
    const int tid = threadIdx.x;
    if (tid < LSR_ORD_NB) cnt[tid] = 0u;
    __syncthreads();
    auto key = [&](int i) { return min((int)((lcount[lo + i] + 15u) >> 4), LSR_ORD_NB - 1); };
    constexpr int STEP = LSR_ORD_THREADS * LSR_ORD_KPT;
    int kr[LSR_ORD_KPT];
    for (int c = 0; c < len; c += STEP) {
#pragma unroll
        for (int j = 0; j < LSR_ORD_KPT; j++) {
            const int i = c + tid + LSR_ORD_THREADS * j;
            kr[j] = i < len ? key(i) : -1;
        }
#pragma unroll
        for (int j = 0; j < LSR_ORD_KPT; j++)
            if (kr[j] >= 0) atomicAdd(&cnt[kr[j]], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // range offsets, heaviest bucket first: one wave's prefix sum (lane k: bucket 63 - k)
        static_assert(LSR_ORD_NB == 64, "one bucket per lane");
        const uint32_t v = cnt[63 - tid];
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(incl, d, 64);
            if (tid >= d) incl += u;
        }
        cnt[63 - tid] = (uint32_t)lo + incl - v;
    }
    __syncthreads();
    for (int c = 0; c < len; c += STEP) {
        if (len > STEP) {   // (one pass holds the whole range otherwise)
#pragma unroll
            for (int j = 0; j < LSR_ORD_KPT; j++) {
                const int i = c + tid + LSR_ORD_THREADS * j;
                kr[j] = i < len ? key(i) : -1;
            }
        }
#pragma unroll
        for (int j = 0; j < LSR_ORD_KPT; j++)
            if (kr[j] >= 0) {
                const uint32_t blk = (uint32_t)(lo + c + tid + LSR_ORD_THREADS * j);
                border[atomicAdd(&cnt[kr[j]], 1u)] =
                    make_uint4(blk, tile_start[blk >> 2], tile_start[(blk >> 2) + 1], lcount[blk]);
            }
    }
}

hipError_t launch_bwd_order(const RenderArgs& a, uint4* border, hipStream_t st)
{
    const int n = 4 * a.cam.gx * a.cam.gy;
    if (n == 0) return hipSuccess;
    k_bwd_order<<<8, LSR_ORD_THREADS, 0, st>>>(a.lcount, a.tile_start, n, border);
    return hipGetLastError();
}

// --------------------------------------------------------- backward -------
// Gradient row width: the compiled channel set's value count, padded to the
// 32-value reduction groups.
int grad_row_width(int D)
{
    const int nl = lang_set_for(D);
    const int nv = LSR_GROW_LANG + (nl > 0 ? nl : 0);
    return (nv + 31) / 32 * 32;
}

// ------------------------------------------------ factorised backward ----
// Every per-(pixel, instance) gradient term is a product of a per-pair
// scalar and a per-pixel quantity, so the pixel sums of a wave are GEMMs:
//   colour / language:  g[j][c]  = sum_p aT[j][p] * dL/dout[c][p]
//   geometry:           with u = dL/dalpha * G, dx = X_j - lx_p (X_j, lx_p
//                       relative to the 8x8 block centre), the six values
//                       (mean2D x/y, conic a/b/c, opacity) are linear in the
//                       moments  sum_p u[j][p] * {1, lx, ly, lx^2, lx*ly, ly^2}
//   per-pair dot:       dot[j][p] = sum_c f[j][c] * dL/dout[c][p]
// All three run on exact-f32 MFMA (v_mfma_f32_16x16x4_f32) over groups of 16
// instances; the serial per-pixel recurrence (T recovery, rec) is the only
// per-pair VALU work left.  The B operands (dL/dout in two layouts and the
// pixel moments) are per-wave constants held in registers.
template <int NL>
struct BwdFrags {
    static constexpr int C = 3 + NL;
    static constexpr int KS = (C + 3) / 4;      // dot K-steps over channels
    static constexpr int NBC = (C + 15) / 16;   // channel blocks of the gradient product
    float dotB[KS][4];    // dL/dout[4t + (l>>4)][pb*16 + (l&15)]
    float chB[NBC][16];   // dL/dout[nb*16 + (l&15)][4t + (l>>4)]
    float momB[16];       // moment (l&15) of block pixel 4t + (l>>4)
};

template <int NL>
__device__ __forceinline__ float gd_at(const RenderBwdArgs& b, int c, int q, int bx, int by)
{
    const Cam& cm = b.f.cam;
    const int qx = bx + (q & 7), qy = by + (q >> 3);
    const bool ok = qx < cm.W && qy < cm.H && c < 3 + b.f.D;
    const size_t HW = (size_t)cm.H * cm.W;
    const size_t pix = (size_t)min(qy, cm.H - 1) * cm.W + min(qx, cm.W - 1);
    const float* src = c < 3 ? b.dout_color + (size_t)c * HW : b.dout_lang + (size_t)min(c - 3, max(b.f.D - 1, 0)) * HW;
    if (c >= 3 && b.f.D == 0) src = b.dout_color;
    const float v = src[pix];
    return ok ? v : 0.f;
}

#ifndef LSR_GRP_STRIDE
#define LSR_GRP_STRIDE 66   // dot/u and aT tiles: conflict-free A-fragment reads (li*66 mod 32 = 2 li)
#endif
#define LSR_BUF_OOB 0x7ffffffc  // a byte offset past every buffer the backward addresses this way
#define LSR_MOM9_STRIDE 12  // reduced moment + colour sums per candidate (16-B aligned rows)
#define LSR_LOG2E 1.4426950408889634f
#define LSR_MF_ATOMIC(ptr, v) atomicAdd((ptr), (v))

// Lane mask of |v| < bound, straight from the compare (the compiler otherwise
// round-trips a ballot's operand through a VGPR: two extra VALU per use).
__device__ __forceinline__ uint64_t lanes_abs_lt(float v, float bound)
{
    uint64_t m;
    asm("v_cmp_gt_f32_e64 %0, %1, |%2|" : "=s"(m) : "s"(bound), "v"(v));
    return m;
}

// Per-wave LDS staging of one chunk's candidate geometry (no feature rows).
// 80 entries: up to 15 candidates carried over from the previous chunk + 64.
// B.w holds the candidate's tile-list position (int bits) once staged: the
// cut extents it carried are only needed by the staging test itself.
struct WaveStageG {
    float4 A[80];
    float4 B[80];
    uint32_t gid[80];
};

// LST: the block's candidate list (written by the forward, RenderArgs::listA/B)
// copied into LDS by LDS-DMA, one 16-candidate group per chunk, two buffers
// (the next chunk lands while this one is processed).  B = {conic.c, opacity,
// id bits, 0-based position bits}.  16-entry chunks keep the D = 16 kernel's
// LDS at 10240 B, which with <= 128 VGPRs (amdgpu_waves_per_eu(4) below) lets
// 4 waves per SIMD reside instead of 3 (64-entry chunks: 12096 B): backward
// 0.503 -> 0.469 ms at cfg3.
#define LSR_LST_CHUNK 16
struct WaveStageL {
    float4 A[2 * LSR_LST_CHUNK];
    float4 B[2 * LSR_LST_CHUNK];
};
// waves per SIMD the MFMA backward is compiled for: 4 for the list-driven
// D = 16 kernel (the headline's), the launch-bounds floor otherwise
template <int NL, bool LD, bool LST, bool DET = false>
constexpr int bwd_waves() { return (LST && LD && NL == 16 && !DET) ? LSR_BWD16_WAVES : LSR_MF_WAVES; }

// LDS-DMA of one 16-B row part per lane: lane l's bytes land at lds + 16 l (an
// LDS-DMA writes wave-uniform M0 + lane x size).  Inline asm with M0 saved and
// restored (the builtin form crashed ROCm 7.2's SIFixSGPRCopies in the quick
// kernel); the caller waits with s_waitcnt vmcnt before reading lds.
__device__ __forceinline__ void glds16(const void* g, const void* lds)
{
    const uint32_t l = (uint32_t)(uintptr_t)lds;   // the LDS byte address (low half of the flat address)
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(l) : "memory");
}

// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt[3:0] bits 3:0, [5:4] bits 15:14;
// expcnt and lgkmcnt at their maxima)
template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N <= 63, "vmcnt is 6 bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");   // also a compiler barrier for the LDS reads after it
}

// Appends this chunk's candidates after the `carry` entries already staged.
__device__ __forceinline__ int stage_candidates_geo(WaveStageG& st, int carry, bool valid, uint32_t gid, int pos,
                                                    int bx, int by, const float4* __restrict__ splatA,
                                                    const float4* __restrict__ splatB)
{
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    if (valid) {
        A = splatA[gid];
        B = splatB[gid];
    }
    const bool ok = valid && block_overlap(A.x, A.y, __float_as_uint(B.w), bx, by) &&
                    block_overlap_exact(A.x, A.y, A.z, A.w, B.x, B.z, bx, by);
    const uint64_t m = wave_ballot(ok);
    if (ok) {
        const int r = carry + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        st.A[r] = A;
        st.B[r] = make_float4(B.x, B.y, B.z, __int_as_float(pos));
        st.gid[r] = gid;
    }
    wave_lds_fence();
    return __popcll(m);
}

// As stage_candidates_geo, with the chunk's records already loaded.
__device__ __forceinline__ int stage_candidates_geo_rec(WaveStageG& st, int carry, bool valid, uint32_t gid, int pos,
                                                        int bx, int by, float4 A, float4 B)
{
    const bool ok = valid && block_overlap(A.x, A.y, __float_as_uint(B.w), bx, by) &&
                    block_overlap_exact(A.x, A.y, A.z, A.w, B.x, B.z, bx, by);
    const uint64_t m = wave_ballot(ok);
    if (ok) {
        const int r = carry + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        st.A[r] = A;
        st.B[r] = make_float4(B.x, B.y, B.z, __int_as_float(pos));
        st.gid[r] = gid;
    }
    wave_lds_fence();
    return __popcll(m);
}

// Feature c of Gaussian gid (rgb, then dense language; 0 past the channels).
template <int NL>
__device__ __forceinline__ float feature_at(const RenderArgs& a, uint32_t gid, int c)
{
    const bool ok = c < 3 + a.D;
    const float* src = c < 3 ? a.rgb + 3 * (size_t)gid + c
                             : (ok ? a.lang + (size_t)gid * a.D + (c - 3) : a.rgb + 3 * (size_t)gid);
    const float v = *src;
    return ok ? v : 0.f;
}

// Channel of the dot product's K-step t in lane group lg.  Default: channel
// 4t + lg.  VEC (whole 16-channel language rows, D = NL, rows 16-B aligned):
// the K order follows the rows' float4 layout, so a candidate's features are
// gathered with one 16-B load per 16-channel line and lane group (lane group
// lg takes float4 lg of each line: K-steps 4r..4r+3 are line r's channels
// 16r + 4lg + u) plus one load of its colour (the last K-step: channel lg,
// lane group 3 none).  The dot is the same sum over channels in another order.
template <int NL, bool VEC>
__device__ __forceinline__ int dot_channel(int t, int lg)
{
    if constexpr (VEC) {
        if (t < NL / 4) return 3 + 16 * (t >> 2) + 4 * lg + (t & 3);
        return lg < 3 ? lg : 3 + NL;   // past the channels: 0
    }
    return 4 * t + lg;
}

// The dot product's A fragments of candidate gid for lane group lg, in
// dot_channel order.
template <int NL, bool VEC, int KS>
__device__ __forceinline__ void dot_features(const RenderArgs& a, uint32_t gid, int lg, float (&af)[KS])
{
    if constexpr (VEC) {
        static_assert(NL % 16 == 0 && KS == NL / 4 + 1, "VEC: whole 16-channel lines");
        const float4* row = reinterpret_cast<const float4*>(a.lang) + (size_t)gid * (NL / 4) + lg;
#pragma unroll
        for (int r = 0; r < NL / 16; r++) {
            const float4 v = row[4 * r];
            af[4 * r + 0] = v.x;
            af[4 * r + 1] = v.y;
            af[4 * r + 2] = v.z;
            af[4 * r + 3] = v.w;
        }
        const float c = a.rgb[3 * (size_t)gid + min(lg, 2)];
        af[NL / 4] = lg < 3 ? c : 0.f;
    } else {
#pragma unroll
        for (int t = 0; t < KS; t++) af[t] = feature_at<NL>(a, gid, 4 * t + lg);
    }
}

#define BWD_MFMA(a, b_, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b_), (c), 0, 0, 0)

// LO (language only): the autograd call needs dL/dlanguage alone (feature-mode
// training: geometry frozen, scene/gaussian_model.py:238-243, and means2D not
// requiring grad).  Then dL/dlang[j][c] = sum_p aT[j][p] dL/dout[c][p] is all
// that is left: no dot products, no dL/dalpha recurrence, no moments, and the
// rows go straight into the (N, D) output (b.grad_acc, b.VP = D).

// SP (with LO): the language input is the quick path's sparse (weights,
// codes) rows; the per-channel gradient rows are gathered at each Gaussian's
// codes into dL/dweights (b.qw_acc, (P, K)) instead of being added densely.
// LST: the candidates come from the forward's per-block list (RenderArgs::listA,
// lcount) instead of being re-staged from the tile list: no ids -> records
// gathers, no block tests, no compaction; the list chunks arrive by LDS-DMA one
// chunk ahead.  The same candidates in the same order: results unchanged.
// DET: the per-block partials are added as 64-bit fixed-point integers
// (render_det.h: det_add at det_shift's exponents) instead of float atomics.
// BA (with LD, not DET: the headline's kernel): the launcher has checked that
// every gradient byte offset fits the buffer atomics' 31 bits, so the 64-bit
// global-atomic fallback is not compiled into the group loop.  LD's row
// strides (VP = 16, D = NL) are compile-time constants: shifts and adds.
template <int NL, bool LO = false, bool LD = false, bool SP = false, bool LST = false, bool DET = false, bool BA = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(bwd_waves<NL, LD, LST, DET>()))) k_render_bwd_mf(RenderBwdArgs b)
{
    static_assert(!BA || (LD && !DET), "BA: the direct-dL/dlang float-atomic backward");
    static_assert(!(LST && SP), "the sparse-input backward follows the quick forward (no lists)");
    static_assert(!(DET && SP), "the deterministic backward expands the sparse input (lsr_api backward_quick)");
    static_assert(!LO || NL > 0, "language-only backward needs D > 0");
    static_assert(!SP || LO, "the sparse-input gradient is a language-only backward");
    static_assert(!LD || (!LO && NL % 16 == 0), "direct dL/dlang needs whole 16-channel lines");
    using FR = BwdFrags<NL>;
    constexpr int KS = FR::KS;
    // LD implies D == NL (launch_render_bwd) and 16-B aligned rows (lsr_api.hip plan_backward)
    constexpr bool VEC = LD;
    // RREG (direct dL/dlang): the language lines' atomics take their values
    // straight from the MFMA accumulators, lane (li, lg) adding candidate
    // 4 lg + q's channel li (the C layout), so those rows skip LDS
    // (LO, not SP: every line is a language line, so all of them come
    // straight from the accumulators and the LDS row tile is not used)
    constexpr bool RREG = LD || (LO && !SP && LSR_BWD_LO_RREG);
    // MFMA channel blocks cover the language channels only; RGB (3) and the
    // six geometry moments are summed on the VALU (see phase 3)
    constexpr int NBC = (NL + 15) / 16;
    constexpr int NBA = NBC > 0 ? NBC : 1;
    __shared__ float2 sRG[64];        // dL/dout R, G of the block's pixels
    __shared__ float sBc[64];         // dL/dout B
    constexpr int GS = LSR_GRP_STRIDE;
    // the stage: re-staged tile-list candidates (!LST) or two list chunks (LST)
    __shared__ std::conditional_t<LST, WaveStageL, WaveStageG> stv;
    auto& st = stv;    // !LST
    auto& stl = stv;   // LST
    // first language column of a staged row; LD: the language lines start at
    // 16 and go to b.lang_acc, the first line (geometry + colour) to the row
    constexpr int GCOL0 = LO ? 0 : (LD ? 16 : LSR_GROW_LANG);
    constexpr int GRL = (GCOL0 + NL + 15) / 16;            // 16-float lines per gradient row
    constexpr int GRS = 16 * GRL + 4;                     // staged row stride
    // The gradient-row tile and the moments are written only after phase 3
    // has read dot/u and aT into registers (a wave's LDS operations complete
    // in order), so they share those buffers: 2.3-5.4 KB less LDS per wave,
    // 12 instead of 10 resident waves per CU at D = 16.
    constexpr int DUG = (16 * GS > 16 * GRS) ? 16 * GS : 16 * GRS;
    __shared__ float sDU[DUG];        // dot[k][p] -> u[k][p] -> the group's gradient rows
    __shared__ __attribute__((aligned(16))) float sAT[16 * GS];   // G[k][p] (phase 1) -> aT[k][p] (phase 2) -> moments
    static_assert(16 * LSR_MOM9_STRIDE <= 16 * GS, "moment rows must fit the aT tile");
    float* const sGr = sDU;
    float* const sMom = sAT;

    const RenderArgs& a = b.f;
    const Cam& c = a.cam;
    const WaveTile wt(a, LST ? a.border : nullptr);
    const int lane = threadIdx.x;
    const int lg = lane >> 4, li = lane & 15;
    const PixMap pm(c, wt.tile, lane + (wt.sub << 6));
    const bool inside = pm.px < c.W && pm.py < c.H;
    const float pfx = (float)pm.px, pfy = (float)pm.py;
    const float cx = (float)pm.bx + 3.5f, cy = (float)pm.by + 3.5f;
    const uint32_t rs = wt.ent ? wt.rs : a.tile_start[wt.tile];
    const size_t HW = (size_t)c.H * c.W;
    const size_t pix = (size_t)pm.py * c.W + pm.px;
    // LD: D == NL (launch_render_bwd) and 16-value rows (plan_backward)
    const int D = (LD && LSR_BWD_LD_STATIC) ? NL : a.D;
    const int VP = (LD && LSR_BWD_LD_STATIC) ? 16 : b.VP;
    const float ddelx_dx = 0.5f * (float)c.W, ddely_dy = 0.5f * (float)c.H;
    // gradient rows (and LD: the language output) as raw buffers when every
    // byte offset fits 31 bits (uniform; otherwise 64-bit global atomics)
    const uint64_t nbg = (uint64_t)a.P * (uint64_t)VP * 4u;
    const uint64_t nbl = LD ? (uint64_t)a.P * (uint64_t)D * 4u : 0u;
    const bool buf_atom = BA || (nbg < (uint64_t)LSR_BUF_OOB && nbl < (uint64_t)LSR_BUF_OOB);
    const __amdgpu_buffer_rsrc_t rg =
        __builtin_amdgcn_make_buffer_rsrc(b.grad_acc, 0, (int)min(nbg, (uint64_t)LSR_BUF_OOB), 0x00020000);
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(
        LD ? b.lang_acc : b.grad_acc, 0, (int)min(LD ? nbl : nbg, (uint64_t)LSR_BUF_OOB), 0x00020000);

    const float T_final = inside ? a.final_T[pix] : 0.f;
    const int last = inside ? (int)a.n_contrib[pix] : 0;
    const int wmax = wave_max_i(last);
    if (wmax == 0) return;
    // Prologue order: the loads the first chunk's staging depends on (ids,
    // then records) are issued before the block's dL/dout fragments, so
    // waiting for them (vector-memory operations complete in issue order)
    // never waits for the 40 fragment loads; the lane's own RGB dL/dout is
    // loaded first among those, reaches LDS (sRG, sBc) just before the chunk
    // loop, and gives the background term without reloading it.
    // SPF: chunk c's ids are loaded two chunks ahead and its records one chunk
    // ahead, so staging never waits on a dependent gather (9 more VGPRs: off
    // for the widest language set, where they would spill)
    constexpr bool SPF = LSR_BWD_SPLAT_PF && NL <= 32;
    // tile-list position clamped to the range (wmax >= 1: position 0 exists), result selected
    auto pl_at = [&](int q) -> uint32_t { const uint32_t v = a.point_list[rs + max(q, 0)]; return q >= 0 ? v : 0u; };
    uint32_t gid1 = 0u, gid2 = 0u;
    float4 A1 = make_float4(0.f, 0.f, 0.f, 0.f), B1 = A1;
    // LST: entries [lbase, lbase + cnt) of the block's list, back to front
    const uint32_t lcnt = LST ? (wt.ent ? wt.lc : a.lcount[4 * wt.tile + wt.sub]) : 0u;
    const size_t lbase = LST ? (size_t)4 * rs + (size_t)wt.sub * ((wt.ent ? wt.re : a.tile_start[wt.tile + 1]) - rs) : 0;
    if constexpr (!LST) {
        gid1 = pl_at(wmax - 1 - lane);
        if constexpr (SPF) {
            gid2 = pl_at(wmax - 65 - lane);
            A1 = a.splatA[gid1];   // gid 0 for positions past the range: a valid record, never staged
            B1 = a.splatB[gid1];
        }
        // entries past a group's end are read unconditionally (immediate-offset
        // loads, no index clamps): keep them finite
        for (int e = lane; e < 80; e += 64) {
            st.A[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            st.B[e] = make_float4(0.f, 0.f, 0.f, __int_as_float(0x7fffffff));
            st.gid[e] = 0u;
        }
    }
    // LST: chunk c0's entries lbase + lcnt - 1 - (c0 + lane) -> stl buffer `off`,
    // lanes < LSR_LST_CHUNK (lanes past the list copy entry 0: finite, and
    // past the group's end)
    auto list_dma = [&](int c0, int off) {
        const int e = (int)lcnt - 1 - (c0 + lane);
        const size_t src = lbase + (size_t)(e >= 0 ? e : 0);
        if (lane < LSR_LST_CHUNK) {
            glds16(a.listA + src, stl.A + off);
            glds16(a.listB + src, stl.B + off);
        }
    };

    float dr0 = 0.f, dr1 = 0.f, dr2 = 0.f;   // the lane's own pixel's RGB dL/dout (0 outside the image)
    if constexpr (!LO) {
        dr0 = gd_at<NL>(b, 0, lane, pm.bx, pm.by);
        dr1 = gd_at<NL>(b, 1, lane, pm.bx, pm.by);
        dr2 = gd_at<NL>(b, 2, lane, pm.bx, pm.by);
    }
    float dotB[KS][4], chB[NBA][16];
    // VEC: the dL/dout fragments through raw buffer descriptors when every
    // byte offset fits 31 bits (uniform): a fragment's offset is its
    // channel's plane plus the pixel's, and a pixel outside the image gets an
    // offset past both buffers (the load returns 0), so no clamps or selects
    const uint64_t HW4 = (uint64_t)HW * 4u;
    const bool gd_buf = VEC && HW4 * (uint64_t)(D > 3 ? D : 3) < 0x7fffffffull;
    if (VEC && gd_buf) {
        const __amdgpu_buffer_rsrc_t rcol = __builtin_amdgcn_make_buffer_rsrc((void*)b.dout_color, 0, (int)(HW4 * 3u), 0x00020000);
        const __amdgpu_buffer_rsrc_t rlng = __builtin_amdgcn_make_buffer_rsrc((void*)b.dout_lang, 0, (int)(HW4 * (uint64_t)D), 0x00020000);
        const uint32_t hw4 = (uint32_t)HW4;
        auto poff = [&](int q) -> uint32_t {
            const int qx = pm.bx + (q & 7), qy = pm.by + (q >> 3);
            return (qx < c.W && qy < c.H) ? (uint32_t)(qy * c.W + qx) * 4u : 0x80000000u;
        };
        auto ld = [&](__amdgpu_buffer_rsrc_t r, uint32_t off) {
            return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
        };
        uint32_t pa[4];
#pragma unroll
        for (int pb = 0; pb < 4; pb++) pa[pb] = poff(pb * 16 + li);
#pragma unroll
        for (int t = 0; t < KS; t++)
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                if (t < NL / 4) {
                    const int chl = dot_channel<NL, VEC>(t, lg) - 3;   // a language channel
                    dotB[t][pb] = ld(rlng, (uint32_t)chl * hw4 + pa[pb]);
                } else {   // colour channel lg; lane group 3 none
                    dotB[t][pb] = ld(rcol, lg < 3 ? (uint32_t)lg * hw4 + pa[pb] : 0x80000000u);
                }
            }
#pragma unroll
        for (int nb = 0; nb < NBC; nb++)
#pragma unroll
            for (int t = 0; t < 16; t++) chB[nb][t] = ld(rlng, (uint32_t)(nb * 16 + li) * hw4 + poff(4 * t + lg));
    } else
    {
    if constexpr (!LO) {
#pragma unroll
        for (int t = 0; t < KS; t++)
#pragma unroll
            for (int pb = 0; pb < 4; pb++)
                dotB[t][pb] = gd_at<NL>(b, dot_channel<NL, VEC>(t, lg), pb * 16 + li, pm.bx, pm.by);
    }
#pragma unroll
    for (int nb = 0; nb < NBC; nb++)
#pragma unroll
        for (int t = 0; t < 16; t++)
            chB[nb][t] = gd_at<NL>(b, 3 + nb * 16 + li, 4 * t + lg, pm.bx, pm.by);
    }
    // block-centred x of the pixels this lane's fragments cover: columns lg
    // (even K-steps) and 4 + lg (odd K-steps)
    const float lxe = (float)lg - 3.5f, lxo = (float)lg + 0.5f;
    const float lxe2 = lxe * lxe, lxo2 = lxo * lxo;
    const float bg0 = c.bg[0], bg1 = c.bg[1], bg2 = c.bg[2];
    // dr* are the lane's own pixel's values (0 outside): 0 with a black
    // background, and the term below is then exact 0
    const float bg_dot = LO ? 0.f : bg0 * dr0 + bg1 * dr1 + bg2 * dr2;

    const bool has_bg = (bg0 != 0.f) || (bg1 != 0.f) || (bg2 != 0.f);   // uniform
    float T = T_final;
    float S = 0.f;

    // positions [0, wmax) back to front, 64 per chunk; candidates are processed
    // in groups of 16, a partial group carried into the next chunk
    int carry = 0;
    float af[KS];
    if constexpr (!LO) {
        sRG[lane] = make_float2(dr0, dr1);
        sBc[lane] = dr2;
    }
    // LST: a chunk's DMA is waited for with vmcnt(N), N = a lower bound of the
    // VMEM operations the previous (full, one-group) chunk issued after it --
    // its buffer atomics, GRL x 4 per group (unconditional, never merged; the
    // feature gathers are not counted) -- so the wait does not drain them
    // INVARIANT: the atomic loop below issues exactly GRL x 4
    // unconditional buffer atomics per group (masked lanes get an out-of-range
    // offset, never a branch), all after this chunk's DMA; the counted wait
    // relies on it.  Change that loop and this count together.
    constexpr int ATOMICS_PER_GROUP = GRL * 4;
    constexpr int OPG = ATOMICS_PER_GROUP;
    constexpr int CGR = LSR_LST_CHUNK / 16;   // groups per list chunk
    constexpr int CHUNK_OPS = CGR * OPG < 63 ? CGR * OPG : 63;
    constexpr int CH = LST ? LSR_LST_CHUNK : 64;   // candidates per chunk
    if constexpr (LST) list_dma(0, 0);
    const int cend = LST ? (int)lcnt : wmax;
    for (int c0 = 0; c0 < cend; c0 += CH) {
        int n, nfull;
        const float4* SA;
        const float4* SB;
        const uint32_t* SG;
        if constexpr (LST) {
            const int off = (c0 / CH & 1) * CH;
            // (DET: conditional 64-bit atomics, so no count of them: drain)
            if (c0 == 0 || !buf_atom || DET) wait_vmcnt<0>();
            else wait_vmcnt<CHUNK_OPS>();
            if (c0 + CH < cend) list_dma(c0 + CH, CH - off);
            n = nfull = min(CH, cend - c0);
            SA = stl.A + off;
            SB = stl.B + off;
            SG = reinterpret_cast<const uint32_t*>(stl.B + off) + 2;   // B.z, stride 4 words
        } else {
            const int p = wmax - 1 - (c0 + lane);
            const bool valid = p >= 0;
            if constexpr (SPF) {
                const uint32_t gid = gid1;
                const float4 Ac = A1, Bc = B1;
                gid1 = gid2;
                A1 = a.splatA[gid1];
                B1 = a.splatB[gid1];
                gid2 = pl_at(p - 128);
                n = carry + stage_candidates_geo_rec(st, carry, valid, gid, p, pm.bx, pm.by, Ac, Bc);
            } else {
                const uint32_t gid = gid1;
                gid1 = pl_at(p - 64);
                n = carry + stage_candidates_geo(st, carry, valid, gid, p, pm.bx, pm.by, a.splatA, a.splatB);
            }
            nfull = (c0 + 64 >= wmax) ? n : (n & ~15);
            SA = st.A;
            SB = st.B;
            SG = st.gid;
        }
        constexpr int SGS = LST ? 4 : 1;   // word stride of the id array

        for (int g0 = 0; g0 < nfull; g0 += 16) {
            const int kn = min(16, nfull - g0);
            // A fragments of the dot product: feature 4t+lg of candidate g0+li,
            // gathered now, consumed after phase 1
            if constexpr (!LO) {
                const uint32_t gi = SG[SGS * (g0 + (li < kn ? li : 0))];
                dot_features<NL, VEC>(a, gi, lg, af);
            }
            // phase 1: G of the 16 candidates (0 where the pair does not
            // contribute), independent across candidates; straight-line code.
            // The forward's exponent cut (power < B.z) needs no test here: below
            // it alpha < e^-0.02 / 255, far outside the fast exp's error band, so
            // the alpha test rejects those pairs.  Lanes in the band are collected
            // as a lane mask (scalar ORs), not per-lane flags.
            uint64_t near_m = 0u;
            const int kn_u = __builtin_amdgcn_readfirstlane(kn);   // uniform: scalar compares below
            // candidate li's opacity in lane li: phase 2 takes candidate k's
            // from lane k (v_readlane) instead of a broadcast LDS read per k
            const int opl = __float_as_int(SB[g0 + li].y);
#define BWD_OP(k) __int_as_float(__builtin_amdgcn_readlane(opl, (k)))
            // GREG: G stays in registers from phase 1 to phase 2 (no LDS round trip)
            float Gr[16];
            (void)Gr;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const float4 A = SA[g0 + k];
                const float4 B = SB[g0 + k];
                const float power = splat_power(A.z, A.w, B.x, A.x - pfx, A.y - pfy);
                const bool cj = (k < kn_u) && (__float_as_int(B.w) < last) && !(power > 0.0f);
                // G = 0 for a non-candidate pair: alpha - 1/255 is then far below the band
                const float G = cj ? __builtin_amdgcn_exp2f(power * LSR_LOG2E) : 0.f;
                const float d = fminf(0.99f, B.y * G) - (1.0f / 255.0f);
                near_m |= lanes_abs_lt(d, 2e-8f);
                Gr[k] = d >= 0.f ? G : 0.f;
            }
            if (near_m != 0u) {
                // the 1/255 decision must be the forward's: lanes inside the fast
                // exp's error band re-evaluate with the forward's exp (rare)
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    if (k >= kn) break;
                    const int j = g0 + k;
                    const float4 A = SA[j];
                    const float4 B = SB[j];
                    const float power = splat_power(A.z, A.w, B.x, A.x - pfx, A.y - pfy);
                    const bool cj = (__float_as_int(B.w) < last) & !(power > 0.0f) & (LST || !(power < B.z));
                    const float af2 = fminf(0.99f, B.y * __builtin_amdgcn_exp2f(power * LSR_LOG2E));
                    if (cj & (fabsf(af2 - (1.0f / 255.0f)) < 2e-8f)) {
                        const float G = expf_det(power);
                        const float alpha = fminf(0.99f, B.y * G);
                        Gr[k] = !(alpha < 1.0f / 255.0f) ? G : 0.f;
                    }
                }
            }
            // dot[k][p] of the group's candidates on MFMA: (16 x C) . (C x 64)
            float dv[16];
            (void)dv;
            if constexpr (!LO) {
                f32x4 acc[4];
#pragma unroll
                for (int pb = 0; pb < 4; pb++) acc[pb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < KS; t++)
#pragma unroll
                    for (int pb = 0; pb < 4; pb++)
                        acc[pb] = BWD_MFMA(af[t], dotB[t][pb], acc[pb]);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    uint32_t x0 = __float_as_uint(acc[0][r]), x1 = __float_as_uint(acc[1][r]);
                    uint32_t x2 = __float_as_uint(acc[2][r]), x3 = __float_as_uint(acc[3][r]);
                    auto s02 = __builtin_amdgcn_permlane32_swap(x0, x2, false, false);
                    auto s13 = __builtin_amdgcn_permlane32_swap(x1, x3, false, false);
                    auto s01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
                    auto s23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
                    dv[0 + r] = __uint_as_float(s01[0]);
                    dv[4 + r] = __uint_as_float(s01[1]);
                    dv[8 + r] = __uint_as_float(s23[0]);
                    dv[12 + r] = __uint_as_float(s23[1]);
                }
            }
            wave_lds_fence();
            // phase 2: the serial back-to-front recurrence per pixel.  S is the
            // colour accumulated behind the current instance (the upstream
            // "accum_rec" once the last contributor is folded in):
            //   dL/dalpha_k = (dot_k - S) T_k,   S <- alpha_k dot_k + (1 - alpha_k) S
            // G = 0 marks a non-contributing pair: alpha = 0, rcp(1) = 1 and the
            // S update is an exact identity, so no selects are needed.
            if constexpr (LO) {
                // transmittance only: aT_k = alpha_k T_k (T_k recovered back to front)
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const float G = Gr[k];
                    const float al = fminf(0.99f, BWD_OP(k) * G);
                    T = T * __builtin_amdgcn_rcpf(1.f - al);
                    sAT[k * GS + lane] = al * T;
                }
            } else if (has_bg) {
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const float G = Gr[k];
                    const float dot = dv[k];
                    const float al = fminf(0.99f, BWD_OP(k) * G);
                    const float om = 1.f - al;
                    const float rcp = __builtin_amdgcn_rcpf(om);
                    T = T * rcp;
                    const float dL_dalpha = fmaf(-T_final * rcp, bg_dot, (dot - S) * T);
                    sDU[k * GS + lane] = dL_dalpha * G;
                    sAT[k * GS + lane] = al * T;
                    S = fmaf(al, dot, om * S);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const float G = Gr[k];
                    const float dot = dv[k];
                    const float al = fminf(0.99f, BWD_OP(k) * G);
                    const float om = 1.f - al;
                    T = T * __builtin_amdgcn_rcpf(om);
                    sDU[k * GS + lane] = ((dot - S) * T) * G;
                    sAT[k * GS + lane] = al * T;
                    S = fmaf(al, dot, om * S);
                }
            }
            wave_lds_fence();
            // phase 3: language gradients on MFMA; RGB gradients and the six
            // pixel moments sum_p u {1, lx, ly, lx^2, lx ly, ly^2} on the VALU.
            // Lane (li, lg) reads candidate li's aT and u at pixel q = 4t + lg
            // (the MFMA A fragments) and keeps partial sums over its 16 pixels;
            // the four lane groups are then added.  Rows pair K-steps 2r
            // (columns lg) and 2r + 1 (columns 4 + lg) at ly = r - 3.5.
            f32x4 ch[NBA];
#pragma unroll
            for (int nb = 0; nb < NBA; nb++) ch[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
            float M0 = 0.f, M1 = 0.f, M2 = 0.f, M3 = 0.f, M4 = 0.f, M5 = 0.f;
            float C0 = 0.f, C1 = 0.f, C2 = 0.f;
            float ue = 0.f;
            if constexpr (LO) {
#pragma unroll
                for (int t = 0; t < 16; t++) {
                    const float aa = sAT[li * GS + 4 * t + lg];
#pragma unroll
                    for (int nb = 0; nb < NBC; nb++) ch[nb] = BWD_MFMA(aa, chB[nb][t], ch[nb]);
                }
            } else {
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const float au = sDU[li * GS + 4 * t + lg];
                const float aa = sAT[li * GS + 4 * t + lg];
#pragma unroll
                for (int nb = 0; nb < NBC; nb++) ch[nb] = BWD_MFMA(aa, chB[nb][t], ch[nb]);
                // (R, G) as one 8-B read + B as a 4-B read: 2 + 2 LDS cycles, where
                // the 12-B read of a float4's three used components (ds_read_b96) costs 8
                const float2 rg = sRG[4 * t + lg];
                const float4 d = make_float4(rg.x, rg.y, sBc[4 * t + lg], 0.f);
                C0 = fmaf(aa, d.x, C0);
                C1 = fmaf(aa, d.y, C1);
                C2 = fmaf(aa, d.z, C2);
                // lx is a lane constant per column parity (lxe even t, lxo odd t)
                // and ly a constant per t, so the six moments follow from the
                // column-parity sums of u, ly u and ly^2 u (3 VALU per t instead
                // of 11 per t pair; combined with lxe / lxo after the loop)
                const float ly = (float)(t >> 1) - 3.5f;
                if ((t & 1) == 0) {
                    M0 += au;
                    M2 = fmaf(ly, au, M2);
                    M5 = fmaf(ly * ly, au, M5);
                } else {
                    M1 += au;
                    M3 = fmaf(ly, au, M3);
                    M4 = fmaf(ly * ly, au, M4);
                }
            }
            {
                // (M0, M2, M5) = even-column sums of (u, ly u, ly^2 u); (M1, M3, M4) the odd columns'
                const float se = M0, so = M1, ye = M2, yo = M3, qe = M5, qo = M4;
                M0 = se + so;
                M1 = fmaf(lxe, se, lxo * so);
                M2 = ye + yo;
                M3 = fmaf(lxe2, se, lxo2 * so);
                M4 = fmaf(lxe, ye, lxo * yo);
                M5 = qe + qo;
            }
            // The nine partial sums over the four lane groups, reduced two at a
            // time: a permlane swap exchanges half of one value for half of
            // another, so swap + add halves two values' lane groups at once
            // (8 swaps + 8 adds instead of 18 xor-exchanges).  Row lg then holds
            // value slot s0(lg) of Y0 and 4 + s0(lg) of Y1 (slots: M0..M5, C0..C2);
            // the rows park them in the moment area (sAT is free once the loop
            // above has read it: a wave's LDS operations complete in order).
            {
                auto red32 = [](float x, float y) {
                    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
                };
                auto red16 = [](float x, float y) {
                    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
                };
                const float Y0 = red16(red32(M0, M1), red32(M2, M3));   // rows: M0 M2 M1 M3
                const float Y1 = red16(red32(M4, M5), red32(C0, C1));   // rows: M4 C0 M5 C1
                const float X4 = red32(C2, C2);
                const float Y2 = red16(X4, X4);                         // row 0: C2
                const int s0 = ((lg & 1) << 1) | (lg >> 1);
                float* const mr = sMom + li * LSR_MOM9_STRIDE;
                mr[s0] = Y0;
                mr[4 + s0] = Y1;
                if (lg == 0) mr[8] = Y2;
            }
            }
            // Gradient rows of the group staged in LDS (row layout of lsr_device.h:
            // [0..5] geometry, [6..8] colour, [12..) language), then added with
            // line-coalesced atomics: each 16-lane group covers one 64-B line of
            // one Gaussian's row.  Language: lane holds slot 4*lg+r, channel nb*16+li.
#pragma unroll
            for (int nb = 0; nb < (RREG ? 0 : NBC); nb++) {
                const int chn = nb * 16 + li;
                if (chn < NL) {
#pragma unroll
                    for (int r = 0; r < 4; r++) sGr[(4 * lg + r) * GRS + GCOL0 + chn] = ch[nb][r];
                }
            }
            if constexpr (!LO) wave_lds_fence();
            if (!LO && lane < kn) {   // lane = candidate li (lg = 0)
                const int j = g0 + lane;
                const float4 A = SA[j];
                const float4 B = SB[j];
                const float* const mr = sMom + lane * LSR_MOM9_STRIDE;
                const float4 m03 = *reinterpret_cast<const float4*>(mr);
                const float4 m47 = *reinterpret_cast<const float4*>(mr + 4);
                const float S0 = m03.x, S1 = m03.y, S2 = m03.z, S3 = m03.w, S4 = m47.x, S5 = m47.y;
                C0 = m47.z;
                C1 = m47.w;
                C2 = mr[8];
                const float X = A.x - cx, Y = A.y - cy;
                const float Sdx = fmaf(X, S0, -S1), Sdy = fmaf(Y, S0, -S2);
                const float Sdxx = fmaf(X, fmaf(X, S0, -2.f * S1), S3);
                const float Sdxy = fmaf(X, fmaf(Y, S0, -S2), fmaf(-Y, S1, S4));
                const float Sdyy = fmaf(Y, fmaf(Y, S0, -2.f * S2), S5);
                const float o = B.y;
                float* gr = sGr + lane * GRS;
                gr[0] = -o * ddelx_dx * fmaf(A.z, Sdx, A.w * Sdy);
                gr[1] = -o * ddely_dy * fmaf(B.x, Sdy, A.w * Sdx);
                gr[2] = -0.5f * o * Sdxx;
                gr[3] = -o * Sdxy;
                gr[4] = -0.5f * o * Sdyy;
                gr[5] = S0;
                gr[6] = C0;
                gr[7] = C1;
                gr[8] = C2;
            }
            wave_lds_fence();
            if constexpr (SP) {
                // (slot, code) pairs: dL/dw[gid][m] += row[slot][idx[gid][m]]
                const int K = a.K;
                for (int e = lane; e < 16 * K; e += 64) {
                    const int slot = e / K, m = e - slot * K;
                    if (slot < kn) {
                        const size_t off = (size_t)SG[SGS * (g0 + slot)] * K + m;
                        const int q = quick_index(a.qi, a.qidx_dtype, off);
                        if (q >= 0 && q < D) {
                            const float v = sGr[slot * GRS + GCOL0 + q];
                            if (v != 0.f) LSR_MF_ATOMIC(b.qw_acc + off, v);
                        }
                    }
                }
            } else {
                // every value and id the group's atomics need is read from LDS
                // first (one wait), then the atomics issue back to back
                uint32_t gq[4];
                float vq[GRL][4];
                // slot of the q-th atomic of this lane: 4q + lg, or (RREG) 4 lg + q
                auto slot_of = [&](int q) { return RREG ? 4 * lg + q : 4 * q + lg; };
#pragma unroll
                for (int q = 0; q < 4; q++) gq[q] = SG[SGS * (g0 + slot_of(q))];
#pragma unroll
                for (int h = 0; h < GRL; h++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (RREG && LO)
                            vq[h][q] = ch[h][q];
                        else if (RREG && h > 0)
                            vq[h][q] = ch[h - 1][q];
                        else
                            vq[h][q] = sGr[slot_of(q) * GRS + 16 * h + li];
                    }
                if constexpr (DET) {
                    // fixed-point twins of the rows (det_shift above): the same
                    // values, order-independent sums
                    uint32_t* const dflag = reinterpret_cast<uint32_t*>(b.det_bounds + 2);
                    uint32_t sq[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) sq[q] = slot_of(q) < kn ? b.det_sh[gq[q]] : 0u;
#pragma unroll
                    for (int h = 0; h < GRL; h++) {
                        const int f = 16 * h + li;
                        const bool fcol = LO ? (f < D)
                                          : LD ? (h == 0 ? (f < 9) : (f - 16 < D))
                                               : ((f < 9) | ((f >= LSR_GROW_LANG) & (f < LSR_GROW_LANG + D)));
                        const int cls = LO ? 0 : ((LD && h > 0) ? 0 : det_class_of(f));
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float v = vq[h][q];
                            if (fcol & (slot_of(q) < kn) & (v != 0.f)) {
                                const int sh = (int)(int8_t)(sq[q] >> (8 * cls));
                                if (LD && h > 0)
                                    det_add(b.det_lang + (size_t)gq[q] * D + (f - 16), v, sh, dflag);
                                else
                                    det_add(b.det_rows + (size_t)gq[q] * VP + f, v, sh, dflag);
                            }
                        }
                    }
                } else if (buf_atom) {
                    // buffer atomics: 32-bit offsets, and a lane with nothing
                    // to add gets an offset past the buffer (the range check
                    // drops it: tools/micro/buf_oob_atomic.hip) instead of an
                    // exec-masked branch per atomic.  INVARIANT: exactly
                    // ATOMICS_PER_GROUP = GRL x 4 of them, unconditionally (the
                    // LST chunk wait above counts them as vmcnt operations)
                    static_assert(ATOMICS_PER_GROUP == GRL * 4, "the LST wait counts these atomics");
#pragma unroll
                    for (int h = 0; h < GRL; h++) {
                        const int f = 16 * h + li;
                        const bool fcol = LO ? (f < D)
                                          : LD ? (h == 0 ? (f < 9) : (f - 16 < D))
                                               : ((f < 9) | ((f >= LSR_GROW_LANG) & (f < LSR_GROW_LANG + D)));
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float v = vq[h][q];
                            const bool on = fcol & (slot_of(q) < kn) & (v != 0.f);
                            if (LD && h > 0) {
                                const int off = (int)(gq[q] * (uint32_t)D + (uint32_t)(f - 16)) * 4;
                                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, rl, on ? off : LSR_BUF_OOB, 0, 0);
                            } else {
                                const int off = (int)(gq[q] * (uint32_t)VP + (uint32_t)f) * 4;
                                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, rg, on ? off : LSR_BUF_OOB, 0, 0);
                            }
                        }
                    }
                } else if constexpr (!BA)
#pragma unroll
                for (int h = 0; h < GRL; h++) {
                    const int f = 16 * h + li;
                    const bool fcol = LO ? (f < D)
                                      : LD ? (h == 0 ? (f < 9) : (f - 16 < D))
                                           : ((f < 9) | ((f >= LSR_GROW_LANG) & (f < LSR_GROW_LANG + D)));
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float v = vq[h][q];
                        if (fcol & (slot_of(q) < kn) & (v != 0.f)) {
                            if (LD && h > 0)
                                LSR_MF_ATOMIC(b.lang_acc + (size_t)gq[q] * D + (f - 16), v);
                            else
                                LSR_MF_ATOMIC(b.grad_acc + (size_t)gq[q] * VP + f, v);
                        }
                    }
                }
            }
            wave_lds_fence();
        }
        // carry the partial group to the front of the stage
        if constexpr (!LST) {
            carry = n - nfull;
            if (nfull > 0 && lane < carry) {   // source >= 16 > destination: no overlap
                st.A[lane] = st.A[nfull + lane];
                st.B[lane] = st.B[nfull + lane];
                st.gid[lane] = st.gid[nfull + lane];
            }
        }
        wave_lds_fence();
    }
}


// The launchers: the kernel form from the call's arguments (with_lang_set /
// with_bools, render_common.h), one wave per 8x8 block.
// LST: the forward's per-block candidate lists (RenderArgs::listA); DET: fixed-point sums
using BwdKernel = void (*)(RenderBwdArgs);

hipError_t launch_render_bwd_lang(const RenderBwdArgs& b, hipStream_t st)
{
    const int T = b.f.cam.gx * b.f.cam.gy;
    if (T == 0) return hipSuccess;
    if (b.det_rows && (!b.det_bounds || !b.det_sh)) return hipErrorInvalidValue;
    BwdKernel k = nullptr;
    const bool known = with_lang_set<4>(lang_set_for(b.f.D), [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        with_bools([&](auto lst, auto det) { k = k_render_bwd_mf<NL, true, false, false, lst.value, det.value>; },
                   b.f.listA != nullptr, b.det_rows != nullptr);
    });
    if (!known) return hipErrorInvalidValue;
    k<<<4 * T, 64, 0, st>>>(b);
    return hipGetLastError();
}

hipError_t launch_render_bwd_lang_sparse(const RenderBwdArgs& b, hipStream_t st)
{
    const int T = b.f.cam.gx * b.f.cam.gy;
    if (T == 0) return hipSuccess;
    if (!b.qw_acc || !b.f.qi || b.f.K <= 0) return hipErrorInvalidValue;
    BwdKernel k = nullptr;
    const bool known = with_lang_set<4>(lang_set_for(b.f.D), [&](auto nl) {
        k = k_render_bwd_mf<decltype(nl)::value, true, false, true>;
    });
    if (!known) return hipErrorInvalidValue;
    k<<<4 * T, 64, 0, st>>>(b);
    return hipGetLastError();
}

static constexpr bool lang_direct_set(int D) { return D == 16 || D == 32; }
bool bwd_lang_direct(int D)
{
    return lang_direct_set(D);
}

hipError_t launch_render_bwd(const RenderBwdArgs& b, hipStream_t st)
{
    const int T = b.f.cam.gx * b.f.cam.gy;
    if (T == 0) return hipSuccess;
    const bool lst = b.f.listA != nullptr;
    const bool det = b.det_rows != nullptr;
    const bool ld = b.lang_acc != nullptr;   // LD: dL/dlanguage straight into lang_acc (then D == NL)
    if (det && (!b.det_bounds || !b.det_sh || (ld != (b.det_lang != nullptr)))) return hipErrorInvalidValue;
    if (ld && (!bwd_lang_direct(b.f.D) || (uintptr_t)b.f.lang % 16 != 0)) return hipErrorInvalidValue;
    if (ld && LSR_BWD_LD_STATIC && b.VP != 16) return hipErrorInvalidValue;   // the kernel's compile-time row width
    BwdKernel k = nullptr;
    const bool known = with_lang_set(lang_set_for(b.f.D), [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        with_bools([&](auto ldc, auto lstc, auto detc) {
            if constexpr (ldc.value && !detc.value && LSR_BWD_LD_STATIC) {
                // LD: (P, 16) rows and (P, NL) language rows; BA when both fit the buffer atomics' offsets
                const uint64_t nb = (uint64_t)b.f.P * (uint64_t)(NL > 16 ? NL : 16) * 4u;
                if constexpr (lang_direct_set(NL))
                    k = nb < (uint64_t)LSR_BUF_OOB ? k_render_bwd_mf<NL, false, true, false, lstc.value, false, true>
                                                   : k_render_bwd_mf<NL, false, true, false, lstc.value, false>;
            } else if constexpr (!ldc.value || lang_direct_set(NL))
                k = k_render_bwd_mf<NL, false, ldc.value, false, lstc.value, detc.value>;
        }, ld, lst, det);
    });
    if (!known) return hipErrorInvalidValue;
    k<<<4 * T, 64, 0, st>>>(b);
    return hipGetLastError();
}

}  // namespace lsr
