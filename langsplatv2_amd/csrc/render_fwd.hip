// render_fwd.hip — the dense forward render k_render_fwd (colour + up to 64
// dense language channels) with its LDS staging, and launch_render_fwd.
// Work decomposition: render_common.h.
#include "render_common.h"

// The ML blend loop's issue-slot cuts; each is bit-identical to
// its 0 form and can be built out for an A/B (make variant VFLAGS=-DLSR_FWD_..=0).
#ifndef LSR_FWD_EXP4
#define LSR_FWD_EXP4 1   // a group's two packed exponent chains advance in lockstep
#endif
#ifndef LSR_FWD_RGB
#define LSR_FWD_RGB 1    // 16-B RGB reads, scalar (not SLP-packed) RGB accumulation
#endif

namespace lsr {

// expf_det2 (lsr_device.h) of two pairs, statement by statement in lockstep:
// the same operations per half in the same order (bitwise expf_det2), with
// every packed FMA followed by an independent one instead of its dependant.
__device__ __forceinline__ void expf_det2x2(f32x2 x0, f32x2 x1, f32x2& e0, f32x2& e1)
{
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    auto fma2 = [](f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); };
    auto k2 = [](float v) { return f32x2{v, v}; };
    x0 = f32x2{__builtin_amdgcn_fmed3f(x0.x, -87.0f, 1.0e30f), __builtin_amdgcn_fmed3f(x0.y, -87.0f, 1.0e30f)};
    x1 = f32x2{__builtin_amdgcn_fmed3f(x1.x, -87.0f, 1.0e30f), __builtin_amdgcn_fmed3f(x1.y, -87.0f, 1.0e30f)};
    const f32x2 t0 = fma2(x0, k2(1.44269504088896341f), k2(12582912.0f));
    const f32x2 t1 = fma2(x1, k2(1.44269504088896341f), k2(12582912.0f));
    const f32x2 n0 = t0 - k2(12582912.0f), n1 = t1 - k2(12582912.0f);
    f32x2 r0 = fma2(n0, k2(-0.693145751953125f), x0), r1 = fma2(n1, k2(-0.693145751953125f), x1);
    r0 = fma2(n0, k2(-1.428606765330187e-06f), r0);
    r1 = fma2(n1, k2(-1.428606765330187e-06f), r1);
    f32x2 p0 = k2(0x1.6aea1ap-10f), p1 = p0;
    constexpr float cf[6] = {0x1.1267d2p-7f, 0x1.555820p-5f, 0x1.555418p-3f, 0x1.fffffcp-2f, 1.0f, 1.0f};
#pragma unroll
    for (int i = 0; i < 6; i++) {
        p0 = fma2(p0, r0, k2(cf[i]));
        p1 = fma2(p1, r1, k2(cf[i]));
    }
    const u32x2 s0 = (__builtin_bit_cast(u32x2, t0) << 23) + u32x2{0x3f800000u, 0x3f800000u};
    const u32x2 s1 = (__builtin_bit_cast(u32x2, t1) << 23) + u32x2{0x3f800000u, 0x3f800000u};
    e0 = p0 * __builtin_bit_cast(f32x2, s0);
    e1 = p1 * __builtin_bit_cast(f32x2, s1);
}

// Stage one instance's feature row (rgb + dense language) into LDS.
template <int NL, int F4>
__device__ __forceinline__ void stage_features(float4* dst, const float* rgb, const float* lang, int D, uint32_t gid)
{
    float row[F4 * 4];
    row[0] = rgb[3 * gid];
    row[1] = rgb[3 * gid + 1];
    row[2] = rgb[3 * gid + 2];
    if (NL > 0 && D == NL && (NL % 4) == 0) {
        const float4* src = reinterpret_cast<const float4*>(lang + (size_t)gid * NL);
#pragma unroll
        for (int q = 0; q < NL / 4; q++) {
            const float4 v = src[q];
            row[3 + 4 * q] = v.x; row[4 + 4 * q] = v.y; row[5 + 4 * q] = v.z; row[6 + 4 * q] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < NL; k++) row[3 + k] = (k < D) ? lang[(size_t)gid * D + k] : 0.f;
    }
#pragma unroll
    for (int k = 3 + NL; k < F4 * 4; k++) row[k] = 0.f;
#pragma unroll
    for (int q = 0; q < F4; q++) dst[q] = make_float4(row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]);
}

// Forward staging with the candidates' geometry pair-interleaved: entry
// j >> 1, component j & 1, so the blend loop reads candidates (2i, 2i+1) of
// each field with one ds_read_b64 and evaluates both exponents with packed
// f32 instructions (bitwise identical to the scalar ones).
// From 16 language channels up the forward is the ML form (k_render_fwd), and
// the ML form does not stage feature rows in LDS: it gathers the candidates'
// language slices as MFMA operands and stages only their RGB (SF below).
template <int NL>
constexpr bool fwd_ml = NL >= 16;
// SF (the ML form) holds NE = 68 entries: up to 3 candidates of a partial
// group carried over from the previous chunk + 64 (with their list positions).
template <int F4, bool SF>
struct WaveStageP {
    static constexpr int NE = SF ? 68 : 64;
    f32x2 X[NE / 2], Y[NE / 2], CA[NE / 2], CB[NE / 2], CC[NE / 2], OP[NE / 2];
    float4 F[SF ? 1 : 64 * F4];
    uint32_t gid[SF ? NE : 1];
    float4 R[SF ? NE : 1];   // SF: the candidates' RGB (read by the ML blend as one broadcast line)
    uint32_t pos[SF ? NE : 1];   // SF: the entry's 1-based list position
    uint8_t src[SF ? 1 : 64];    // !SF: the staging lane (position = chunk base + src + 1)
};

// The backward's per-block candidate list (RenderArgs::listA/B): with LST the
// staged candidates are also written to list entries [lpos, lpos + cnt) in
// staging order (increasing tile-list position), B as {conic.c, opacity, id,
// 0-based position}; *mo receives the chunk's staging mask.
struct ListSink {
    float4* A = nullptr;
    float4* B = nullptr;
    uint32_t pos = 0;
};

template <int NL, int F4, bool LST = false>
__device__ __forceinline__ int stage_candidates_p_rec(WaveStageP<F4, fwd_ml<NL>>& st, bool valid, uint32_t gid,
                                                      int pos, int bx, int by, float4 A, float4 B,
                                                      const float* __restrict__ rgb, const float* __restrict__ lang,
                                                      int D, const ListSink& ls = ListSink(), uint64_t* mo = nullptr,
                                                      int off = 0)
{
    constexpr bool SF = fwd_ml<NL>;
    constexpr int NE = WaveStageP<F4, SF>::NE;
    const bool ok = valid && block_overlap(A.x, A.y, __float_as_uint(B.w), bx, by) &&
                    block_overlap_exact(A.x, A.y, A.z, A.w, B.x, B.z, bx, by);
    const uint64_t m = wave_ballot(ok);
    const int cnt = __popcll(m);
    if constexpr (LST) *mo = m;
    if (ok) {
        const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if constexpr (LST) {
            if (ls.A) {
                ls.A[ls.pos + r] = A;
                ls.B[ls.pos + r] = make_float4(B.x, B.y, __uint_as_float(gid), __int_as_float(pos - 1));
            }
        }
        // entry i = off + r (SF: after the carried entries)
        const int i = off + r;
        float* base = reinterpret_cast<float*>(&st) + (i & 1);
        const int e = (i >> 1) * 2;
        base[0 * NE + e] = A.x;
        base[1 * NE + e] = A.y;
        base[2 * NE + e] = A.z;
        base[3 * NE + e] = A.w;
        base[4 * NE + e] = B.x;
        base[5 * NE + e] = B.y;
        if constexpr (SF) {
            st.pos[i] = (uint32_t)pos;
            st.gid[i] = gid;
            st.R[i] = make_float4(rgb[3 * (size_t)gid], rgb[3 * (size_t)gid + 1], rgb[3 * (size_t)gid + 2], 0.f);
        } else {
            st.src[r] = (uint8_t)(threadIdx.x & 63);
        }
        if constexpr (!SF)
            stage_features<NL, F4>(&st.F[r * F4], rgb, lang, D, gid);
    }
    wave_lds_fence();
    return cnt;
}

template <int NL, int F4, bool LST = false>
__device__ __forceinline__ int stage_candidates_p(WaveStageP<F4, fwd_ml<NL>>& st, bool valid, uint32_t gid, int pos, int bx,
                                                  int by, const float4* __restrict__ splatA,
                                                  const float4* __restrict__ splatB, const float* __restrict__ rgb,
                                                  const float* __restrict__ lang, int D, const ListSink& ls = ListSink(),
                                                  uint64_t* mo = nullptr, int off = 0)
{
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    if (valid) {
        A = splatA[gid];
        B = splatB[gid];
    }
    return stage_candidates_p_rec<NL, F4, LST>(st, valid, gid, pos, bx, by, A, B, rgb, lang, D, ls, mo, off);
}

// The backward's accumulators (RenderArgs::zero; lsr_fwd_out.grad_ws): a
// grid-strided share per wave, non-temporal 16-B stores, issued first so no
// early exit skips them.  The render is VALU / LDS bound; these writes replace
// the backward's two memset launches.
__device__ __forceinline__ void zero_backward_accumulators(const RenderArgs& a)
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    const size_t stride = (size_t)gridDim.x * 64;
    if (a.zero) {
        v4f* const z = reinterpret_cast<v4f*>(a.zero);
        for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < a.zero_n16; i += stride)
            __builtin_nontemporal_store(v4f{0.f, 0.f, 0.f, 0.f}, z + i);
    }
    if (a.zero2) {
        v4f* const z = reinterpret_cast<v4f*>(a.zero2);
        for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < a.zero2_n16; i += stride)
            __builtin_nontemporal_store(v4f{0.f, 0.f, 0.f, 0.f}, z + i);
    }
}

// ZERO: this launch also clears the backward's accumulators (a.zero set);
// a separate instantiation, so a forward without a pending backward runs the
// unchanged kernel (the clearing loop alone moved cfg5's D = 32 render by +2 %)
// ML (D > 16): the language channels accumulate on the matrix
// cores instead of the VALU.  Per 4 staged candidates the blend (alpha, the
// serial transmittance / termination recurrence, the RGB sums) runs per pixel
// lane as below; the 4 x 64 weights aT are transposed in registers (two
// permlane swaps per pair of rows: lane group <-> candidate) into the B
// operand of v_mfma_f32_16x16x4_f32, whose A operand is each 16-channel
// block of the 4 candidates' language rows (gathered per lane; their RGB is
// staged in LDS with the candidate).  The MFMA is bitwise a fmaf chain over
// its 4 K terms in order (tools/micro/mfma_order.hip) and a skipped pair has
// aT = 0, so the outputs are bit-identical to the per-lane sequential blend;
// the VALU no longer issues the 2 x D language FMAs per candidate pair, which
// run on the otherwise idle matrix pipe.  (The LDS-staged-row form, D = 16,
// measured slower than the VALU blend and is not launched.)
// MLM (with ML): D below the language set's width NL (masked channels);
// otherwise D == NL is a compile-time constant (fewer registers).
// the D = 16 ML form at 6 waves / SIMD (80 VGPRs): its blend is latency bound
template <int NL, bool ML>
constexpr int fwd_waves() { return (ML && NL == 16) ? 6 : 1; }
template <int NL, bool ZERO = false, bool ML = false, bool MLM = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(fwd_waves<NL, ML>()))) k_render_fwd(RenderArgs a)
{
    if constexpr (ZERO) zero_backward_accumulators(a);
    constexpr int C = 3 + NL;
    constexpr int F4 = (C + 3) / 4;  // float4 per feature row
    constexpr bool SF = fwd_ml<NL>;
    static_assert(!ML || NL == 16 || NL == 32 || NL == 64, "ML: whole 16-channel language blocks");
    // gathered rows feed the ML form only, and the ML form's carried partial
    // groups and `last` are kept in the SF stage (st.pos / st.gid / st.R): a
    // build with ML but LDS-staged rows would drop them
    static_assert(ML == SF, "the ML form and the SF stage go together (NL >= 16)");
    constexpr int MLB = ML ? NL / 16 : 1;   // ML: 16-channel output blocks
    __shared__ WaveStageP<F4, SF> st;

    const Cam& c = a.cam;
    const WaveTile wt(a);
    const int lane = threadIdx.x;
    const PixMap pm(c, wt.tile, lane + (wt.sub << 6));
    const bool inside = pm.px < c.W && pm.py < c.H;
    const float pfx = (float)pm.px, pfy = (float)pm.py;
    const uint32_t rs = a.tile_start[wt.tile], re = a.tile_start[wt.tile + 1];
    const int D = (ML && !MLM) ? NL : a.D;

    float T = 1.0f;
    bool done = !inside;
    float acc[F4 * 4];
#pragma unroll
    for (int k = 0; k < F4 * 4; k++) acc[k] = 0.f;
    f32x4 mlacc[MLB][4];   // ML: lane (li, lg) holds language channels 16 nb + 4 lg + r of block pixel 16 pb + li
#pragma unroll
    for (int nb = 0; nb < MLB; nb++)
#pragma unroll
        for (int pb = 0; pb < 4; pb++) mlacc[nb][pb] = f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t last = 0;

    // ZERO (a backward is pending): the staged candidates also go to this
    // block's list for the backward (RenderArgs::listA), nst entries so far;
    // (mlast, nlast, blast): the last chunk's mask, entries before it, its start
    ListSink ls;
    uint32_t nst = 0, nlast = 0, blast = rs;
    uint64_t mlast = 0;
    if constexpr (ZERO) {
        if (a.listA) {
            ls.A = a.listA + (size_t)4 * rs + (size_t)wt.sub * (re - rs);
            ls.B = a.listB + (size_t)4 * rs + (size_t)wt.sub * (re - rs);
        }
    }
    uint32_t next_gid = (rs + lane < re) ? a.point_list[rs + lane] : 0u;
    // SPF: a chunk's ids are loaded two chunks ahead and its records one chunk
    // ahead, issued after the current chunk's feature loads: the staging then
    // waits for one dependent gather (the feature rows) instead of two.
    // Positions past the list read gid 0 (a valid record, never staged).
    // (not with gathered feature rows, the ML form: cfg5 1.73 -> 1.82 ms)
    constexpr bool FSPF = !SF;
    uint32_t next_gid2 = 0u;
    float4 A1 = make_float4(0.f, 0.f, 0.f, 0.f), B1 = A1;
    if (FSPF && rs < re) {
        next_gid2 = (rs + 64 + lane < re) ? a.point_list[rs + 64 + lane] : 0u;
        A1 = a.splatA[next_gid];
        B1 = a.splatB[next_gid];
    }
    // ML: a partial group (carry < 4 entries) waits in the stage for the next
    // chunk's candidates, so every group but the list's last is full: the
    // blend's per-group work is paid per 4 candidates, not per chunk remainder.
    // The blend is per candidate in list order either way (bit-identical).
    int carry = 0;
    for (uint32_t base = rs; base < re; base += 64) {
        if (wave_ballot(!done) == 0) break;
        const uint32_t idx = base + lane;
        const bool valid = idx < re;
        const uint32_t gid = next_gid;
        int n;
        uint64_t mchunk = 0;
        ls.pos = nst;
        if constexpr (FSPF) {
            const float4 Ac = A1, Bc = B1;
            n = stage_candidates_p_rec<NL, F4, ZERO>(st, valid, gid, (int)(idx - rs) + 1, pm.bx, pm.by, Ac, Bc, a.rgb,
                                                     a.lang, D, ls, &mchunk, ML ? carry : 0);
            next_gid = next_gid2;
            A1 = a.splatA[next_gid];
            B1 = a.splatB[next_gid];
            const uint32_t q = min(idx + 128, re - 1);   // re > base: a valid position
            const uint32_t v = a.point_list[q];
            next_gid2 = idx + 128 < re ? v : 0u;
        } else {
            next_gid = (idx + 64 < re) ? a.point_list[idx + 64] : 0u;
            n = stage_candidates_p<NL, F4, ZERO>(st, valid, gid, (int)(idx - rs) + 1, pm.bx, pm.by, a.splatA,
                                                 a.splatB, a.rgb, a.lang, D, ls, &mchunk, ML ? carry : 0);
        }
        if constexpr (ZERO) {
            mlast = mchunk;
            nlast = nst;
            blast = base;
            nst += (uint32_t)n;
        }
        // Two instances per iteration, branch-free per lane: a lane that
        // skips an instance (exponent cut, alpha < 1/255, saturated or done)
        // blends it with weight 0 and keeps T.  The two exp chains are
        // independent (ILP); T carries from the first to the second exactly
        // as in the sequential per-pixel order.
        int lastj = -1;   // LASTJ: staged index of the chunk's last contributor
        if constexpr (ML) {
            const int lg = lane >> 4, li = lane & 15;
            const float* const Fs = reinterpret_cast<const float*>(st.F);
            n += carry;   // the stage's entries: carried + this chunk's
            // full groups only, except in the list's last chunk
            const int nproc = (base + 64 >= re) ? n : (n & ~3);
            int q0 = 0;
            for (; q0 < nproc; q0 += 4) {
                if (wave_ballot(!done) == 0) break;
                // A operand: language channel 16 nb + li of candidate q0 + lg
                // (0 past the chunk) -- from the staged rows, or (SF) gathered
                float av[MLB];
#pragma unroll
                for (int nb = 0; nb < MLB; nb++) {
                    // MLM: channels past D (a language set wider than D) read 0
                    const int ch = 16 * nb + li;
                    float fa;
                    if constexpr (SF)
                        fa = a.lang[(size_t)st.gid[min(q0 + lg, n - 1)] * D + (MLM ? min(ch, D - 1) : ch)];
                    else
                        fa = Fs[(q0 + lg) * (F4 * 4) + 3 + ch];
                    av[nb] = ((q0 + lg < n) & (!MLM || ch < D)) ? fa : 0.f;
                }
                // al[k]: the pair's alpha where it is blended (the lane not done,
                // exponent <= 0, alpha >= 1/255), else 0; cm[k] the lanes of al != 0
                float al[4];
                bool cm[4];
                f32x2 EX4[2];
                (void)EX4;
                if constexpr (LSR_FWD_EXP4) {
                    f32x2 P4[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int e = (q0 >> 1) + h;
                        const f32x2 dx = st.X[e] - f32x2{pfx, pfx}, dy = st.Y[e] - f32x2{pfy, pfy};
                        P4[h] = __builtin_elementwise_fma(f32x2{-0.5f, -0.5f},
                                                          __builtin_elementwise_fma(st.CA[e] * dx, dx, (st.CC[e] * dy) * dy),
                                                          -((st.CB[e] * dx) * dy));
                    }
                    expf_det2x2(P4[0], P4[1], EX4[0], EX4[1]);
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int j0 = q0 + 2 * h, e = j0 >> 1;
                    const f32x2 sX = st.X[e], sY = st.Y[e], sCA = st.CA[e], sCB = st.CB[e], sCC = st.CC[e];
                    const f32x2 OP = st.OP[e];
                    const f32x2 dx = sX - f32x2{pfx, pfx}, dy = sY - f32x2{pfy, pfy};
                    const f32x2 P = __builtin_elementwise_fma(f32x2{-0.5f, -0.5f},
                                                              __builtin_elementwise_fma(sCA * dx, dx, (sCC * dy) * dy),
                                                              -((sCB * dx) * dy));
                    const f32x2 EX = LSR_FWD_EXP4 ? EX4[h] : expf_det2(P);
                    const float a0 = fminf(0.99f, OP.x * EX.x), a1 = fminf(0.99f, OP.y * EX.y);
                    // no exponent-cut test: below the cut the 1/255 test rejects the pair
                    const bool c0 = (j0 < n) & !done & !(P.x > 0.0f) & !(a0 < 1.0f / 255.0f);
                    const bool c1 = (j0 + 1 < n) & !done & !(P.y > 0.0f) & !(a1 < 1.0f / 255.0f);
                    al[2 * h] = c0 ? a0 : 0.f;
                    al[2 * h + 1] = c1 ? a1 : 0.f;
                    cm[2 * h] = c0;
                    cm[2 * h + 1] = c1;
                }
                // the serial recurrence.  T never increases, so if no lane's
                // transmittance after the 4 candidates (computed as if none
                // terminated) is below 1e-4, none terminated: then a lane with
                // al = 0 gets aT = 0 and T unchanged with no selects and no
                // termination tests.  Otherwise (rare) the group runs the legacy
                // ok0 / term / ok logic.  Bitwise the legacy result either way.
                float s4[4];
                // candidate k's rgb (past the chunk a staged row's: aT = 0 there)
                auto rgb_of = [&](int k) -> float3 {
                    const int kk = min(q0 + k, n - 1);
                    if constexpr (SF) {   // the line staged with the candidate
                        const float4 f = st.R[kk];
                        // keep the 16-B read (ds_read_b128: 4 LDS cycles, the narrowed b96: 8)
                        if constexpr (LSR_FWD_RGB) asm volatile("" ::"v"(f.w));
                        return make_float3(f.x, f.y, f.z);
                    } else {
                        const float4 f = st.F[kk * F4];
                        return make_float3(f.x, f.y, f.z);
                    }
                };
                // transmittance before each candidate, assuming no termination
                float Tk[5];
                Tk[0] = T;
#pragma unroll
                for (int k = 0; k < 4; k++) Tk[k + 1] = Tk[k] * (1.0f - al[k]);
                if (wave_ballot(Tk[4] < 0.0001f) == 0u) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float aT = al[k] * Tk[k];
                        const float3 f = rgb_of(k);
                        acc[0] = fmaf(f.x, aT, acc[0]);
                        acc[1] = fmaf(f.y, aT, acc[1]);
                        acc[2] = fmaf(f.z, aT, acc[2]);
                        // three scalar chains: packed into v_pk_fma_f32 they need register
                        // shuffles, and packed f32 beside the MFMAs costs more than it saves
                        if constexpr (LSR_FWD_RGB) asm("" : "+v"(acc[1]), "+v"(acc[2]));
                        lastj = cm[k] ? q0 + k : lastj;
                        s4[k] = aT;
                    }
                    T = Tk[4];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float alk = al[k];
                        const float test_T = T * (1.0f - alk);
                        const bool ok0 = (alk != 0.f) & !done;
                        const bool term = ok0 & (test_T < 0.0001f);
                        done = done | term;
                        const bool ok = ok0 & !term;
                        const float aT = ok ? alk * T : 0.f;
                        const float3 f = rgb_of(k);
                        acc[0] = fmaf(f.x, aT, acc[0]);
                        acc[1] = fmaf(f.y, aT, acc[1]);
                        acc[2] = fmaf(f.z, aT, acc[2]);
                        T = ok ? test_T : T;
                        lastj = ok ? q0 + k : lastj;
                        s4[k] = aT;
                    }
                }
                // transpose (lane group, candidate): lane (li, lg) then holds
                // candidate lg's aT at block pixel 16 pb + li in s4[pb]
                {
                    auto sw32 = [](float& x, float& y) {
                        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                        x = __uint_as_float(r[0]);
                        y = __uint_as_float(r[1]);
                    };
                    auto sw16 = [](float& x, float& y) {
                        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                        x = __uint_as_float(r[0]);
                        y = __uint_as_float(r[1]);
                    };
                    sw32(s4[0], s4[2]);
                    sw32(s4[1], s4[3]);
                    sw16(s4[0], s4[1]);
                    sw16(s4[2], s4[3]);
                }
#pragma unroll
                for (int pb = 0; pb < 4; pb++)
#pragma unroll
                    for (int nb = 0; nb < MLB; nb++)
                        mlacc[nb][pb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nb], s4[pb], mlacc[nb][pb], 0, 0, 0);
            }
            if constexpr (SF) {
                if (lastj >= 0) last = st.pos[lastj];
                lastj = -1;
                // the partial group's entries [q0, n) -> [0, carry) (q0 >= 4 when
                // they move: no overlap; a wave's LDS accesses complete in order)
                carry = n - q0;
                if (q0 > 0 && carry > 0) {
                    if (lane < carry) {
                        const int i = q0 + lane;
                        float* fb = reinterpret_cast<float*>(&st);
                        constexpr int NE = WaveStageP<F4, SF>::NE;
                        float v[6];
#pragma unroll
                        for (int f = 0; f < 6; f++) v[f] = fb[f * NE + i];
                        const uint32_t pv = st.pos[i], gv = st.gid[i];
                        const float4 rv = st.R[i];
#pragma unroll
                        for (int f = 0; f < 6; f++) fb[f * NE + lane] = v[f];
                        st.pos[lane] = pv;
                        st.gid[lane] = gv;
                        st.R[lane] = rv;
                    }
                }
            }
        } else
        for (int j0 = 0; j0 < n; j0 += 2) {
            if (wave_ballot(!done) == 0) break;
            const bool two = j0 + 1 < n;
            const int j1 = two ? j0 + 1 : j0;
            // both candidates' exponents at once (splat_power, lane-wise);
            // a missing second candidate reads a stale slot: ok1 masks it
            const int e = j0 >> 1;
            const f32x2 sX = st.X[e], sY = st.Y[e], sCA = st.CA[e], sCB = st.CB[e], sCC = st.CC[e];
            const f32x2 OP = st.OP[e];
            const f32x2 dx = sX - f32x2{pfx, pfx}, dy = sY - f32x2{pfy, pfy};
            const f32x2 P = __builtin_elementwise_fma(f32x2{-0.5f, -0.5f},
                                                      __builtin_elementwise_fma(sCA * dx, dx, (sCC * dy) * dy),
                                                      -((sCB * dx) * dy));
            const float p0 = P.x, p1 = P.y;
            // no exponent-cut test: below the cut alpha < e^-0.02 / 255, so the
            // 1/255 test below rejects the pair anyway (exact)
            bool ok0 = !done && !(p0 > 0.0f);
            bool ok1 = two && !done && !(p1 > 0.0f);
            const f32x2 EX = expf_det2(P);   // both exponents packed (bitwise = expf_det)
            const float al0 = fminf(0.99f, OP.x * EX.x);
            const float al1 = fminf(0.99f, OP.y * EX.y);
            ok0 = ok0 && !(al0 < 1.0f / 255.0f);
            ok1 = ok1 && !(al1 < 1.0f / 255.0f);
            {
                const float test_T = T * (1.0f - al0);
                const bool term = ok0 && (test_T < 0.0001f);
                done = done || term;
                ok0 = ok0 && !term;
                ok1 = ok1 && !term;
                const float aT = ok0 ? al0 * T : 0.f;
                {
#pragma unroll
                    for (int f = 0; f < F4; f++) {
                        const float4 v = st.F[j0 * F4 + f];
                        // the row's zero padding past channel C is not accumulated
                        if (4 * f + 0 < C) acc[4 * f + 0] = fmaf(v.x, aT, acc[4 * f + 0]);
                        if (4 * f + 1 < C) acc[4 * f + 1] = fmaf(v.y, aT, acc[4 * f + 1]);
                        if (4 * f + 2 < C) acc[4 * f + 2] = fmaf(v.z, aT, acc[4 * f + 2]);
                        if (4 * f + 3 < C) acc[4 * f + 3] = fmaf(v.w, aT, acc[4 * f + 3]);
                        // keep the 16-B read (ds_read_b128: 4 LDS cycles; the b96 the
                        // compiler would narrow it to costs 8)
                        else asm volatile("" ::"v"(v.w));
                    }
                }
                T = ok0 ? test_T : T;
                lastj = ok0 ? j0 : lastj;
            }
            {
                const float test_T = T * (1.0f - al1);
                const bool term = ok1 && (test_T < 0.0001f);
                done = done || term;
                ok1 = ok1 && !term;
                const float aT = ok1 ? al1 * T : 0.f;
                {
#pragma unroll
                    for (int f = 0; f < F4; f++) {
                        const float4 v = st.F[j1 * F4 + f];
                        // the row's zero padding past channel C is not accumulated
                        if (4 * f + 0 < C) acc[4 * f + 0] = fmaf(v.x, aT, acc[4 * f + 0]);
                        if (4 * f + 1 < C) acc[4 * f + 1] = fmaf(v.y, aT, acc[4 * f + 1]);
                        if (4 * f + 2 < C) acc[4 * f + 2] = fmaf(v.z, aT, acc[4 * f + 2]);
                        if (4 * f + 3 < C) acc[4 * f + 3] = fmaf(v.w, aT, acc[4 * f + 3]);
                        // keep the 16-B read (ds_read_b128: 4 LDS cycles; the b96 the
                        // compiler would narrow it to costs 8)
                        else asm volatile("" ::"v"(v.w));
                    }
                }
                T = ok1 ? test_T : T;
                lastj = ok1 ? j1 : lastj;
            }
        }
        if constexpr (!ML) {
            if (lastj >= 0) last = (uint32_t)(base - rs) + 1u + st.src[lastj];
        }
        wave_lds_fence();
    }
    if constexpr (ZERO) {
        if (a.listA) {
            // entries the backward needs: 0-based position < wmax (the block's largest
            // n_contrib).  Exact when wmax falls in the last staged chunk (the usual
            // case); otherwise every entry before that chunk (the extra ones have
            // position >= every pixel's n_contrib: the backward evaluates them to 0)
            const int wmax = wave_max_i(inside ? (int)last : 0);
            const int off = wmax - (int)(blast - rs);
            uint32_t cnt = nlast;
            if (off > 0) cnt += (uint32_t)__popcll(off >= 64 ? mlast : (mlast & ((1ull << off) - 1ull)));
            if (lane == 0) a.lcount[4 * wt.tile + wt.sub] = cnt;
        }
    }
    if (inside) {
        const size_t HW = (size_t)c.H * c.W;
        const size_t pix = (size_t)pm.py * c.W + pm.px;
        a.final_T[pix] = T;
        a.n_contrib[pix] = last;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) a.out_color[ch * HW + pix] = fmaf(T, c.bg[ch], acc[ch]);
        if constexpr (!ML) {
#pragma unroll
            for (int k = 0; k < NL; k++)
                if (k < D) a.out_lang[k * HW + pix] = acc[3 + k];
        }
    }
    if constexpr (ML) {
        const size_t HW = (size_t)c.H * c.W;
        const int lg = lane >> 4, li = lane & 15;
#pragma unroll
        for (int pb = 0; pb < 4; pb++) {
            const int q = pb * 16 + li;
            const int qx = pm.bx + (q & 7), qy = pm.by + (q >> 3);
            if (qx < c.W && qy < c.H) {
                const size_t pix = (size_t)qy * c.W + qx;
#pragma unroll
                for (int nb = 0; nb < MLB; nb++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (16 * nb + 4 * lg + r < D) a.out_lang[(size_t)(16 * nb + 4 * lg + r) * HW + pix] = mlacc[nb][pb][r];
            }
        }
    }
}

int lang_set_for(int D)
{
    return lang_set_ceil(LangSets{}, D);
}

hipError_t launch_render_fwd(const RenderArgs& a, hipStream_t st)
{
    const int T = a.cam.gx * a.cam.gy;
    if (T == 0) return hipSuccess;
    if (a.qw) return launch_render_fwd_quick(a, st);
    // D <= 8: the VALU blend.  D in (8, 16]: the ML form with gathered rows (cfg3
    // render_fwd 0.307 -> 0.299 ms against the VALU blend; the ML form with
    // LDS-staged rows measured +2.6 %).  D in (16, 32]: cfg5 render_fwd 1.650 ->
    // 1.266 ms.  D in (32, 64]: measured 0.996 -> 0.688 ms against the earlier
    // 16-candidate-group MFMA kernel at cfg3 geometry; the VALU-only blend is
    // slower still.  MLM: D below the set's width.
    void (*k)(RenderArgs) = nullptr;
    const bool known = with_lang_set(lang_set_for(a.D), [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        constexpr bool ML = fwd_ml<NL>;
        with_bools([&](auto zero, auto mlm) {
            if constexpr (ML || !mlm.value) k = k_render_fwd<NL, zero.value, ML, mlm.value>;
        }, a.zero || a.zero2, ML && a.D != NL);
    });
    if (!known) return hipErrorInvalidValue;
    k<<<4 * T, 64, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace lsr
