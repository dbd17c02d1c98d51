// render_quick.hip — the forward render of the sparse "quick" language path
// (K (weight, code) pairs per Gaussian, Dq output channels), three
// generations: k_render_fwd_quick (accumulators in LDS), k_render_fwd_quick_v
// (in registers) and k_render_fwd_quick_d (in registers, chunk rows by
// LDS-DMA).  Work decomposition: render_common.h.
#include "render_common.h"

#define LSR_QUICK_KMAX 12   // quick path: (weight, code) pairs per Gaussian staged with the record

namespace lsr {

// Sparse "quick" language path: Dq output channels, K (weight, index) pairs
// per Gaussian.  One wave per 8x8 pixel block; per-pixel accumulators in LDS
// laid out [channel][lane] (conflict-free: the channel index is wave-uniform
// because every lane processes the same Gaussian).
__global__ void __launch_bounds__(64) k_render_fwd_quick(RenderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = a.K, Dq = a.Dq;
    float* acc = (float*)smem;                                    // Dq * 64
    float4* sA = (float4*)(smem + (size_t)Dq * 64 * 4);           // 64
    float4* sB = sA + 64;                                         // 64
    float* sRGB = (float*)(sB + 64);                              // 64 * 3
    float* sW = sRGB + 64 * 3;                                    // 64 * K
    int* sI = (int*)(sW + 64 * K);                                // 64 * K

    const Cam& c = a.cam;
    const int tile = band_tile(xcd_remap(blockIdx.x >> 2, gridDim.x >> 2), c.gx, c.gy);
    const int t = threadIdx.x;
    const PixMap pm(c, tile, t + ((blockIdx.x & 3) << 6));
    const bool inside = pm.px < c.W && pm.py < c.H;
    const float pfx = (float)pm.px, pfy = (float)pm.py;
    const uint32_t rs = a.tile_start[tile], re = a.tile_start[tile + 1];
    for (int q = 0; q < Dq; q++) acc[q * 64 + t] = 0.f;

    float T = 1.0f, cr = 0.f, cg = 0.f, cb = 0.f;
    uint32_t last = 0;
    bool done = !inside;
    for (uint32_t base = rs; base < re; base += 64) {
        if (__syncthreads_count(done) == 64) break;
        const uint32_t idx = base + t;
        if (idx < re) {
            const uint32_t gid = a.point_list[idx];
            sA[t] = a.splatA[gid];
            sB[t] = a.splatB[gid];
            sRGB[3 * t] = a.rgb[3 * gid];
            sRGB[3 * t + 1] = a.rgb[3 * gid + 1];
            sRGB[3 * t + 2] = a.rgb[3 * gid + 2];
            for (int k = 0; k < K; k++) {
                sW[t * K + k] = a.qw[(size_t)gid * K + k];
                const int q = quick_index(a.qi, a.qidx_dtype, (size_t)gid * K + k);
                sI[t * K + k] = (q >= 0 && q < Dq) ? q : -1;
            }
        }
        __syncthreads();
        const int n = (int)min(64u, re - base);
        const uint32_t pos0 = base - rs + 1;
        bool ok = false;
        if (t < n) ok = block_overlap(sA[t].x, sA[t].y, __float_as_uint(sB[t].w), pm.bx, pm.by);
        uint64_t bits = wave_ballot(ok);
        while (bits) {
            if (wave_ballot(!done) == 0) break;
            const int j = __builtin_ctzll(bits);
            bits &= bits - 1;
            if (done) continue;
            const float4 A = sA[j];
            const float4 B = sB[j];
            const float dx = A.x - pfx, dy = A.y - pfy;
            const float power = splat_power(A.z, A.w, B.x, dx, dy);
            if (power > 0.0f || power < B.z) continue;
            const float G = expf_det(power);
            const float alpha = fminf(0.99f, B.y * G);
            if (alpha < 1.0f / 255.0f) continue;
            const float test_T = T * (1.0f - alpha);
            if (test_T < 0.0001f) {
                done = true;
                continue;
            }
            const float aT = alpha * T;
            cr = fmaf(sRGB[3 * j], aT, cr);
            cg = fmaf(sRGB[3 * j + 1], aT, cg);
            cb = fmaf(sRGB[3 * j + 2], aT, cb);
            for (int k = 0; k < K; k++) {
                const int q = sI[j * K + k];
                if (q >= 0) acc[q * 64 + t] = fmaf(sW[j * K + k], aT, acc[q * 64 + t]);
            }
            T = test_T;
            last = pos0 + j;
        }
    }
    if (inside) {
        const size_t HW = (size_t)c.H * c.W;
        const size_t pix = (size_t)pm.py * c.W + pm.px;
        a.final_T[pix] = T;
        a.n_contrib[pix] = last;
        a.out_color[pix] = fmaf(T, c.bg[0], cr);
        a.out_color[HW + pix] = fmaf(T, c.bg[1], cg);
        a.out_color[2 * HW + pix] = fmaf(T, c.bg[2], cb);
        for (int q = 0; q < Dq; q++) a.out_lang[q * HW + pix] = acc[q * 64 + t];
    }
}

// Quick path, sparse accumulation in registers (default for Dq <= 192, K <= 12).
// The dense-slab kernels above scatter each group's (weight, code) pairs into a
// 16 x Dq tile and accumulate it on MFMA: 16x the arithmetic the 12 non-zero
// codes need, plus barriers between the blend wave and the slab waves.  Here
// one wave per 8x8 block keeps each pixel's Dq accumulators in VGPRs (NP
// vectors of 32) and, per contributing candidate, adds only its K pairs:
// the code is wave-uniform, so acc[code] is a register indexed by M0 (movrel)
// and each pair costs one FMA plus two register moves.  Same per-pixel
// recurrence, same fmaf(w, alpha T, acc) in candidate order as the oracle:
// bit-exact.  Staged per candidate in LDS: the splat record, rgb, the K
// weights and the codes as bytes (0xFF = outside [0, Dq)).
typedef float lsr_f32x32 __attribute__((ext_vector_type(32)));
struct WaveStageV {
    float4 A[64];
    float4 B[64];          // .w = 1-based tile-list position (int bits)
    float4 C[64];          // rgb
    float4 Wt[64][3];      // weights 0..11
    uint4 Q[64];           // codes 0..11 as bytes
};

// The Dq <= 192 accumulators live in v64..v255, outside the compiler's
// allocation (amdgpu_num_vgpr(63): compiled code uses v0..v62; an asm clobber
// of v255 makes the kernel descriptor allocate all 256).  A candidate's K <= 12
// updates run in one asm block in VGPR index mode with SRC2 and DST indexed
// from v63: code q is stored as index q + 1, so v_fma_f32 v63, w, aT, v63
// updates v[64 + q] in one VALU instruction, and an invalid code (index 0)
// lands in the junk register v63.  M0 (the index) is saved and restored.
// (s_set_gpr_idx_idx reads only bits [7:0], so byte k of a code word is
// selected by a shift.)
// The index needs one wait state before the VALU that uses it: the shift
// forming the NEXT code's index (into the other of two SGPRs) fills it, so only
// the word's last code takes an s_nop (3 per candidate instead of 12).
#define LSR_QV_WORD(word, w0, w1, w2, w3)                                               \
    "s_set_gpr_idx_idx %[" #word "]\n\t"                                                \
    "s_lshr_b32 %[ia], %[" #word "], 8\n\t"                                             \
    "v_fma_f32 v63, %[" #w0 "], %[aT], v63\n\t"                                         \
    "s_set_gpr_idx_idx %[ia]\n\t"                                                       \
    "s_lshr_b32 %[ib], %[" #word "], 16\n\t"                                            \
    "v_fma_f32 v63, %[" #w1 "], %[aT], v63\n\t"                                         \
    "s_set_gpr_idx_idx %[ib]\n\t"                                                       \
    "s_lshr_b32 %[ia], %[" #word "], 24\n\t"                                            \
    "v_fma_f32 v63, %[" #w2 "], %[aT], v63\n\t"                                         \
    "s_set_gpr_idx_idx %[ia]\n\t"                                                       \
    "s_nop 0\n\t"                                                                       \
    "v_fma_f32 v63, %[" #w3 "], %[aT], v63\n\t"
// one candidate's K <= 12 pairs (codes in three words q0..q2, weights w0..w11)
#define LSR_QV_UPDATE(aT_, Q_, W0_, W1_, W2_)                                                                   \
    do {                                                                                                        \
        const uint32_t qw0 = __builtin_amdgcn_readfirstlane((Q_).x), qw1 = __builtin_amdgcn_readfirstlane((Q_).y), \
                       qw2 = __builtin_amdgcn_readfirstlane((Q_).z);                                            \
        uint32_t ia, ib, sv;                                                                                    \
        asm volatile("s_mov_b32 %[sv], m0\n\t"                                                                  \
                     "s_set_gpr_idx_on 0, gpr_idx(SRC2,DST)\n\t"                                                \
                     LSR_QV_WORD(q0, w0, w1, w2, w3) LSR_QV_WORD(q1, w4, w5, w6, w7)                            \
                     LSR_QV_WORD(q2, w8, w9, w10, w11)                                                          \
                     "s_set_gpr_idx_off\n\t"                                                                    \
                     "s_mov_b32 m0, %[sv]"                                                                      \
                     : [ia] "=&s"(ia), [ib] "=&s"(ib), [sv] "=&s"(sv)                                           \
                     : [q0] "s"(qw0), [q1] "s"(qw1), [q2] "s"(qw2), [aT] "v"(aT_), [w0] "v"((W0_).x),           \
                       [w1] "v"((W0_).y), [w2] "v"((W0_).z), [w3] "v"((W0_).w), [w4] "v"((W1_).x),              \
                       [w5] "v"((W1_).y), [w6] "v"((W1_).z), [w7] "v"((W1_).w), [w8] "v"((W2_).x),              \
                       [w9] "v"((W2_).y), [w10] "v"((W2_).z), [w11] "v"((W2_).w)                                \
                     : "scc");                                                                                  \
    } while (0)

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // the v255 clobber is the point: it sizes the allocation
template <int NP>
__global__ void __launch_bounds__(64, 2) __attribute__((amdgpu_num_vgpr(63))) k_render_fwd_quick_v(RenderArgs a)
{
    static_assert(NP >= 1 && NP <= 6, "up to 192 quick channels");
    __shared__ WaveStageV st;
    const Cam& c = a.cam;
    const WaveTile wt(a);
    const int lane = threadIdx.x;
    const PixMap pm(c, wt.tile, lane + (wt.sub << 6));
    const bool inside = pm.px < c.W && pm.py < c.H;
    const float pfx = (float)pm.px, pfy = (float)pm.py;
    const uint32_t rs = a.tile_start[wt.tile], re = a.tile_start[wt.tile + 1];
    const int K = a.K, Dq = a.Dq;

    {   // zero v63 (junk) .. v255 (accumulators)
        uint32_t i, sv;
        asm volatile(
            "s_mov_b32 %[sv], m0\n\t"
            "s_mov_b32 %[i], 0\n\t"
            "s_set_gpr_idx_on 0, gpr_idx(DST)\n\t"
            "1:\n\t"
            "s_set_gpr_idx_idx %[i]\n\t"
            "s_nop 0\n\t"
            "v_mov_b32 v63, 0\n\t"
            "s_add_u32 %[i], %[i], 1\n\t"
            "s_cmp_lt_u32 %[i], 193\n\t"
            "s_cbranch_scc1 1b\n\t"
            "s_set_gpr_idx_off\n\t"
            "s_mov_b32 m0, %[sv]"
            : [i] "=&s"(i), [sv] "=&s"(sv)
            :
            : "scc", "v63", "v255", "memory");
    }
    float T = 1.0f, cr = 0.f, cg = 0.f, cbl = 0.f;
    uint32_t last = 0;
    bool done = !inside;
    uint32_t next_gid = (rs + lane < re) ? a.point_list[rs + lane] : 0u;
    for (uint32_t base = rs; base < re; base += 64) {
        if (wave_ballot(!done) == 0) break;
        const uint32_t idx = base + lane;
        const bool valid = idx < re;
        const uint32_t gid = next_gid;
        next_gid = (idx + 64 < re) ? a.point_list[idx + 64] : 0u;
        float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
        if (valid) {
            A = a.splatA[gid];
            B = a.splatB[gid];
        }
        const bool ok = valid && block_overlap(A.x, A.y, __float_as_uint(B.w), pm.bx, pm.by) &&
                        block_overlap_exact(A.x, A.y, A.z, A.w, B.x, B.z, pm.bx, pm.by);
        const uint64_t m = wave_ballot(ok);
        if (ok) {
            const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            st.A[r] = A;
            st.B[r] = make_float4(B.x, B.y, B.z, __int_as_float((int)(idx - rs) + 1));
            st.C[r] = make_float4(a.rgb[3 * (size_t)gid], a.rgb[3 * (size_t)gid + 1], a.rgb[3 * (size_t)gid + 2], 0.f);
            float wv[12];
            uint32_t qv[3] = {0u, 0u, 0u};   // register index q + 1 per code; 0 = the junk register
#pragma unroll
            for (int k = 0; k < 12; k++) {
                wv[k] = 0.f;
                if (k < K) {
                    const size_t off = (size_t)gid * K + k;
                    wv[k] = a.qw[off];
                    const int q = quick_index(a.qi, a.qidx_dtype, off);
                    const uint32_t qb = (q >= 0 && q < Dq) ? (uint32_t)(q + 1) : 0u;
                    qv[k >> 2] |= qb << (8 * (k & 3));
                }
            }
            st.Wt[r][0] = make_float4(wv[0], wv[1], wv[2], wv[3]);
            st.Wt[r][1] = make_float4(wv[4], wv[5], wv[6], wv[7]);
            st.Wt[r][2] = make_float4(wv[8], wv[9], wv[10], wv[11]);
            st.Q[r] = make_uint4(qv[0], qv[1], qv[2], 0u);
        }
        wave_lds_fence();
        const int n = __popcll(m);
        // two candidates per step: their exponents on packed f32 (expf_det2,
        // bitwise = expf_det), then the per-pixel recurrence in order
        for (int j0 = 0; j0 < n; j0 += 2) {
            if (wave_ballot(!done) == 0) break;
            const bool two = j0 + 1 < n;
            const int j1 = two ? j0 + 1 : j0;
            const float4 A0 = st.A[j0], B0 = st.B[j0];
            const float4 A1 = st.A[j1], B1 = st.B[j1];
            const float p0 = splat_power(A0.z, A0.w, B0.x, A0.x - pfx, A0.y - pfy);
            const float p1 = splat_power(A1.z, A1.w, B1.x, A1.x - pfx, A1.y - pfy);
            bool ok0 = !done && !(p0 > 0.0f || p0 < B0.z);
            bool ok1 = two && !done && !(p1 > 0.0f || p1 < B1.z);
            if (!wave_any(ok0 || ok1)) continue;
            const f32x2 EX = expf_det2(f32x2{p0, p1});
            const float al0 = fminf(0.99f, B0.y * EX.x);
            const float al1 = fminf(0.99f, B1.y * EX.y);
            ok0 = ok0 && !(al0 < 1.0f / 255.0f);
            ok1 = ok1 && !(al1 < 1.0f / 255.0f);
            float aT0, aT1;
            {
                const float test_T = T * (1.0f - al0);
                const bool term = ok0 && (test_T < 0.0001f);
                done = done || term;
                ok0 = ok0 && !term;
                ok1 = ok1 && !term;
                aT0 = ok0 ? al0 * T : 0.f;
                if (ok0) {
                    const float4 C0 = st.C[j0];
                    cr = fmaf(C0.x, aT0, cr);
                    cg = fmaf(C0.y, aT0, cg);
                    cbl = fmaf(C0.z, aT0, cbl);
                    T = test_T;
                    last = (uint32_t)__float_as_int(B0.w);
                }
            }
            {
                const float test_T = T * (1.0f - al1);
                const bool term = ok1 && (test_T < 0.0001f);
                done = done || term;
                ok1 = ok1 && !term;
                aT1 = ok1 ? al1 * T : 0.f;
                if (ok1) {
                    const float4 C1 = st.C[j1];
                    cr = fmaf(C1.x, aT1, cr);
                    cg = fmaf(C1.y, aT1, cg);
                    cbl = fmaf(C1.z, aT1, cbl);
                    T = test_T;
                    last = (uint32_t)__float_as_int(B1.w);
                }
            }
            if (wave_any(ok0)) LSR_QV_UPDATE(aT0, st.Q[j0], st.Wt[j0][0], st.Wt[j0][1], st.Wt[j0][2]);
            if (wave_any(ok1)) LSR_QV_UPDATE(aT1, st.Q[j1], st.Wt[j1][0], st.Wt[j1][1], st.Wt[j1][2]);
        }
        wave_lds_fence();
    }
    const size_t HW = (size_t)c.H * c.W;
    if (inside) {
        const size_t pix = (size_t)pm.py * c.W + pm.px;
        a.final_T[pix] = T;
        a.n_contrib[pix] = last;
        a.out_color[pix] = fmaf(T, c.bg[0], cr);
        a.out_color[HW + pix] = fmaf(T, c.bg[1], cg);
        a.out_color[2 * HW + pix] = fmaf(T, c.bg[2], cbl);
        float* const o = a.out_lang + pix;
        for (int q = 0; q < Dq; q++) {
            float v;
            uint32_t sv;
            asm volatile(
                "s_mov_b32 %[sv], m0\n\t"
                "s_set_gpr_idx_on %[q], gpr_idx(SRC0)\n\t"
                "s_nop 0\n\t"
                "v_mov_b32 %[v], v64\n\t"
                "s_set_gpr_idx_off\n\t"
                "s_mov_b32 m0, %[sv]"
                : [v] "=v"(v), [sv] "=&s"(sv)
                : [q] "s"(q)
                : "memory");
            o[(size_t)q * HW] = v;
        }
    }
}
#pragma clang diagnostic pop

// Quick path with the chunk records prefetched by LDS-DMA (default when the
// sparse rows allow 16-B copies: K % 4 == 0, 16-B aligned weights/indices).
// k_render_fwd_quick_v gathers each chunk's records, rgb, 12 weights and 12
// indices into VGPRs when it reaches the chunk, so every chunk waits for two
// dependent global round trips, and at 2 waves/SIMD (the 192 accumulators take
// the register file) nothing hides them (r03 PMC: waves parked in s_waitcnt
// 59 % of their cycles).  Here the NEXT chunk's raw rows are copied straight
// into a per-wave LDS buffer by global_load_lds (no VGPR destination, ids
// loaded two chunks ahead) while the current chunk blends; staging then reads
// LDS.  Blend, accumulation and outputs are k_render_fwd_quick_v's, bit for bit.
// NQ = 16-B parts of an index row: 3 (fp32 / int32), 6 (int64), 1 (packed)
template <int NQ>
struct WaveRawQ {
    float4 A[64];
    float4 B[64];
    float rgb[3][64];                   // channel c of lane l (three 4-B DMAs)
    float4 W[3][64];                    // weight row part p (4 weights) of lane l
    uint4 Q[NQ][64];                    // index row bytes [16 p, 16 p + 16) of lane l
    uint32_t nid[64];                   // the point-list ids of the chunk after next
};
template <int DT>
constexpr int quick_nq() { return DT == 2 ? 6 : DT == 3 ? 1 : 3; }

template <int DT>
__device__ __forceinline__ int quick_code_raw(const WaveRawQ<quick_nq<DT>()>& raw, int lane, int k)
{
    if constexpr (DT == 2) {
        const uint4 q = raw.Q[k >> 1][lane];
        const uint32_t lo = (k & 1) ? q.z : q.x, hi = (k & 1) ? q.w : q.y;
        return hi != 0u || lo > 0x7fffffffu ? -1 : (int)lo;
    } else {
        const uint4 q = raw.Q[k >> 2][lane];
        const uint32_t v = (k & 3) == 0 ? q.x : (k & 3) == 1 ? q.y : (k & 3) == 2 ? q.z : q.w;
        return DT == 0 ? quick_code_f32(__uint_as_float(v)) : (int)v;
    }
}

// One chunk's rows -> raw by LDS-DMA (K = 12 codes per Gaussian): lane l's
// record, rgb, weight row and index row land at slot l of each array (an LDS-
// DMA writes wave-uniform M0 + lane x size).  One asm block walks M0 through
// the arrays (raw's layout is fixed by the static_asserts below); the weight
// and index row parts are the immediate offsets of one address each; the same
// asm block also copies the point-list ids two chunks ahead into raw.nid, so
// no VGPR-destination load is ever in flight behind the DMAs (a compiler-
// inserted wait for such a load is a vmcnt(N) that the compiler computes
// without the asm's DMAs, and drained them: every chunk's first pair waited
// for the prefetch just issued).  The
// immediate offset applies to the LDS destination as well (M0 + offset + 16
// lane), so M0 steps to each array's base minus that offset.  The colour
// goes as three 4-B DMAs (one channel plane each): a dwordx3 LDS-DMA does not
// land at 12 x lane (measured: wrong colours with the 12-B layout).  (The
// __builtin_amdgcn_global_load_lds form crashes ROCm 7.2's SIFixSGPRCopies in
// this kernel, and per-call M0 constants spilled SGPRs.)  The caller waits with
// s_waitcnt vmcnt before reading raw.
#define LSR_GLDS(step, insn) "s_add_u32 m0, m0, " #step "\n\ts_nop 0\n\t" insn "\n\t"
template <int NQ>
__device__ __forceinline__ void quick_dma12(WaveRawQ<NQ>& raw, const RenderArgs& a, uint32_t g, const uint32_t* pI)
{
    static_assert(offsetof(WaveRawQ<NQ>, B) == 1024 && offsetof(WaveRawQ<NQ>, rgb) == 2048 &&
                  offsetof(WaveRawQ<NQ>, W) == 2816 && offsetof(WaveRawQ<NQ>, Q) == 5888 &&
                  offsetof(WaveRawQ<NQ>, nid) == 5888 + 1024 * NQ, "raw layout");
    const uint32_t base = (uint32_t)(uintptr_t)&raw;   // the LDS byte address (low half of the flat address)
    const float4* pA = a.splatA + g;
    const float4* pB = a.splatB + g;
    const float* pR = a.rgb + 3 * (size_t)g;
    const float* pW = a.qw + 12 * (size_t)g;
    const char* pQ = reinterpret_cast<const char*>(a.qi) + (size_t)g * (16 * NQ);
    uint32_t keep;
    if constexpr (NQ == 1) {
        asm volatile("s_mov_b32 %[keep], m0\n\t"
                     "s_mov_b32 m0, %[base]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[pA], off\n\t"
                     LSR_GLDS(1024, "global_load_lds_dwordx4 %[pB], off")
                     LSR_GLDS(1024, "global_load_lds_dword %[pR], off")
                     LSR_GLDS(252, "global_load_lds_dword %[pR], off offset:4")
                     LSR_GLDS(252, "global_load_lds_dword %[pR], off offset:8")
                     LSR_GLDS(264, "global_load_lds_dwordx4 %[pW], off")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pW], off offset:16")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pW], off offset:32")
                     LSR_GLDS(1056, "global_load_lds_dwordx4 %[pQ], off")
                     LSR_GLDS(1024, "global_load_lds_dword %[pI], off")
                     "s_mov_b32 m0, %[keep]"
                     : [keep] "=&s"(keep)
                     : [base] "s"(base), [pA] "v"(pA), [pB] "v"(pB), [pR] "v"(pR), [pW] "v"(pW), [pQ] "v"(pQ),
                       [pI] "v"(pI)
                     : "memory", "scc");
    } else if constexpr (NQ == 3) {
        asm volatile("s_mov_b32 %[keep], m0\n\t"
                     "s_mov_b32 m0, %[base]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[pA], off\n\t"
                     LSR_GLDS(1024, "global_load_lds_dwordx4 %[pB], off")
                     LSR_GLDS(1024, "global_load_lds_dword %[pR], off")
                     LSR_GLDS(252, "global_load_lds_dword %[pR], off offset:4")
                     LSR_GLDS(252, "global_load_lds_dword %[pR], off offset:8")
                     LSR_GLDS(264, "global_load_lds_dwordx4 %[pW], off")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pW], off offset:16")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pW], off offset:32")
                     LSR_GLDS(1056, "global_load_lds_dwordx4 %[pQ], off")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:16")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:32")
                     LSR_GLDS(1056, "global_load_lds_dword %[pI], off")
                     "s_mov_b32 m0, %[keep]"
                     : [keep] "=&s"(keep)
                     : [base] "s"(base), [pA] "v"(pA), [pB] "v"(pB), [pR] "v"(pR), [pW] "v"(pW), [pQ] "v"(pQ),
                       [pI] "v"(pI)
                     : "memory", "scc");
    } else {
        asm volatile("s_mov_b32 %[keep], m0\n\t"
                     "s_mov_b32 m0, %[base]\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %[pA], off\n\t"
                     LSR_GLDS(1024, "global_load_lds_dwordx4 %[pB], off")
                     LSR_GLDS(1024, "global_load_lds_dword %[pR], off")
                     LSR_GLDS(252, "global_load_lds_dword %[pR], off offset:4")
                     LSR_GLDS(252, "global_load_lds_dword %[pR], off offset:8")
                     LSR_GLDS(264, "global_load_lds_dwordx4 %[pW], off")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pW], off offset:16")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pW], off offset:32")
                     LSR_GLDS(1056, "global_load_lds_dwordx4 %[pQ], off")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:16")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:32")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:48")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:64")
                     LSR_GLDS(1008, "global_load_lds_dwordx4 %[pQ], off offset:80")
                     LSR_GLDS(1104, "global_load_lds_dword %[pI], off")
                     "s_mov_b32 m0, %[keep]"
                     : [keep] "=&s"(keep)
                     : [base] "s"(base), [pA] "v"(pA), [pB] "v"(pB), [pR] "v"(pR), [pW] "v"(pW), [pQ] "v"(pQ),
                       [pI] "v"(pI)
                     : "memory", "scc");
    }
}
#undef LSR_GLDS

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // the v255 clobber is the point: it sizes the allocation
// Pixel-major epilogue (LSR_LAYOUT_HWC): the pixel's 192 weights, v64..v255, as 48
// 16-B stores into its 768-B row (immediate offsets from one address).
#define LSR_QHWC(a, b, off) "global_store_dwordx4 %[p], v[" #a ":" #b "], off offset:" #off "\n\t"
#define LSR_QHWC_ALL \
    LSR_QHWC(64, 67, 0) LSR_QHWC(68, 71, 16) LSR_QHWC(72, 75, 32) LSR_QHWC(76, 79, 48) \
    LSR_QHWC(80, 83, 64) LSR_QHWC(84, 87, 80) LSR_QHWC(88, 91, 96) LSR_QHWC(92, 95, 112) \
    LSR_QHWC(96, 99, 128) LSR_QHWC(100, 103, 144) LSR_QHWC(104, 107, 160) LSR_QHWC(108, 111, 176) \
    LSR_QHWC(112, 115, 192) LSR_QHWC(116, 119, 208) LSR_QHWC(120, 123, 224) LSR_QHWC(124, 127, 240) \
    LSR_QHWC(128, 131, 256) LSR_QHWC(132, 135, 272) LSR_QHWC(136, 139, 288) LSR_QHWC(140, 143, 304) \
    LSR_QHWC(144, 147, 320) LSR_QHWC(148, 151, 336) LSR_QHWC(152, 155, 352) LSR_QHWC(156, 159, 368) \
    LSR_QHWC(160, 163, 384) LSR_QHWC(164, 167, 400) LSR_QHWC(168, 171, 416) LSR_QHWC(172, 175, 432) \
    LSR_QHWC(176, 179, 448) LSR_QHWC(180, 183, 464) LSR_QHWC(184, 187, 480) LSR_QHWC(188, 191, 496) \
    LSR_QHWC(192, 195, 512) LSR_QHWC(196, 199, 528) LSR_QHWC(200, 203, 544) LSR_QHWC(204, 207, 560) \
    LSR_QHWC(208, 211, 576) LSR_QHWC(212, 215, 592) LSR_QHWC(216, 219, 608) LSR_QHWC(220, 223, 624) \
    LSR_QHWC(224, 227, 640) LSR_QHWC(228, 231, 656) LSR_QHWC(232, 235, 672) LSR_QHWC(236, 239, 688) \
    LSR_QHWC(240, 243, 704) LSR_QHWC(244, 247, 720) LSR_QHWC(248, 251, 736) LSR_QHWC(252, 255, 752)
// Epilogue of the 192-channel quick kernel: channel q = N - 64 is register vN.
#define LSR_QEPI(N) "buffer_store_dword v" #N ", %[vo], %[rs], %[so] offen\n\ts_add_u32 %[so], %[so], %[hw4]\n\t"
#define LSR_QEPI10(h) LSR_QEPI(h##0) LSR_QEPI(h##1) LSR_QEPI(h##2) LSR_QEPI(h##3) LSR_QEPI(h##4) \
                      LSR_QEPI(h##5) LSR_QEPI(h##6) LSR_QEPI(h##7) LSR_QEPI(h##8) LSR_QEPI(h##9)
#define LSR_QEPI_ALL                                                                                     \
    LSR_QEPI(64) LSR_QEPI(65) LSR_QEPI(66) LSR_QEPI(67) LSR_QEPI(68) LSR_QEPI(69)                        \
    LSR_QEPI10(7) LSR_QEPI10(8) LSR_QEPI10(9) LSR_QEPI10(10) LSR_QEPI10(11) LSR_QEPI10(12) LSR_QEPI10(13) \
    LSR_QEPI10(14) LSR_QEPI10(15) LSR_QEPI10(16) LSR_QEPI10(17) LSR_QEPI10(18) LSR_QEPI10(19)             \
    LSR_QEPI10(20) LSR_QEPI10(21) LSR_QEPI10(22) LSR_QEPI10(23) LSR_QEPI10(24)                           \
    LSR_QEPI(250) LSR_QEPI(251) LSR_QEPI(252) LSR_QEPI(253) LSR_QEPI(254) LSR_QEPI(255)
// BAND: one wave per 16x4 band of the tile (the channel-major map: each of the
// 192 channel stores then writes 64-B row pieces instead of 32-B ones, render
// -2.5 %); else one wave per 8x8 block (the pixel-major map, whose stores are
// per-pixel rows: the tighter block cull wins, -5.6 %)
template <int DT, bool BAND>
__global__ void __launch_bounds__(64, 2) __attribute__((amdgpu_num_vgpr(63))) k_render_fwd_quick_d(RenderArgs a)
{
    constexpr int NQ = quick_nq<DT>();
    __shared__ WaveStageV st;
    __shared__ WaveRawQ<NQ> raw;
    const Cam& c = a.cam;
    const WaveTile wt(a);
    const int lane = threadIdx.x;
    constexpr int BW = BAND ? 16 : 8, BH = 64 / BW;
    PixMap pm(c, wt.tile, lane + (wt.sub << 6));
    if constexpr (BAND) {
        pm.bx = (wt.tile % c.gx) * LSR_TILE;
        pm.by = (wt.tile / c.gx) * LSR_TILE + wt.sub * BH;
        pm.px = pm.bx + (lane & (BW - 1));
        pm.py = pm.by + lane / BW;
    }
    const bool inside = pm.px < c.W && pm.py < c.H;
    const float pfx = (float)pm.px, pfy = (float)pm.py;
    const uint32_t rs = a.tile_start[wt.tile], re = a.tile_start[wt.tile + 1];
    const int Dq = a.Dq;

    {   // zero v63 (junk) .. v255 (accumulators)
        uint32_t i, sv;
        asm volatile(
            "s_mov_b32 %[sv], m0\n\t"
            "s_mov_b32 %[i], 0\n\t"
            "s_set_gpr_idx_on 0, gpr_idx(DST)\n\t"
            "1:\n\t"
            "s_set_gpr_idx_idx %[i]\n\t"
            "s_nop 0\n\t"
            "v_mov_b32 v63, 0\n\t"
            "s_add_u32 %[i], %[i], 1\n\t"
            "s_cmp_lt_u32 %[i], 193\n\t"
            "s_cbranch_scc1 1b\n\t"
            "s_set_gpr_idx_off\n\t"
            "s_mov_b32 m0, %[sv]"
            : [i] "=&s"(i), [sv] "=&s"(sv)
            :
            : "scc", "v63", "v255", "memory");
    }
    float T = 1.0f, cr = 0.f, cg = 0.f, cbl = 0.f;
    uint32_t last = 0;
    bool done = !inside;
    // the first chunk's rows, and (in raw.nid) the ids of the chunk after it; positions
    // past the list read the list's last id, and gid 0 (a valid row, never staged) is used
    if (rs < re) quick_dma12<NQ>(raw, a, (rs + lane < re) ? a.point_list[rs + lane] : 0u,
                                 a.point_list + min(rs + 64 + lane, re - 1));
    for (uint32_t base = rs; base < re; base += 64) {
        if (wave_ballot(!done) == 0) break;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this chunk's rows have landed in raw
        const uint32_t idx = base + lane;
        const bool valid = idx < re;
        const float4 A = raw.A[lane], B = raw.B[lane];
        const bool ok = valid && rect_overlap(A.x, A.y, __float_as_uint(B.w), pm.bx, pm.by, BW - 1, BH - 1) &&
                        rect_overlap_exact(A.x, A.y, A.z, A.w, B.x, B.z, pm.bx, pm.by, (float)(BW - 1), (float)(BH - 1));
        const uint64_t m = wave_ballot(ok);
        if (ok) {
            const int r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            st.A[r] = A;
            st.B[r] = make_float4(B.x, B.y, B.z, __int_as_float((int)(idx - rs) + 1));
            st.C[r] = make_float4(raw.rgb[0][lane], raw.rgb[1][lane], raw.rgb[2][lane], 0.f);
            st.Wt[r][0] = raw.W[0][lane];
            st.Wt[r][1] = raw.W[1][lane];
            st.Wt[r][2] = raw.W[2][lane];
            uint32_t qv[3] = {0u, 0u, 0u};   // register index q + 1 per code; 0 = the junk register
            if constexpr (DT == 3) {
                // packed rows are register indices already; a byte above Dq (not
                // written by lsr_quick_pack_codes for this Dq) is dropped, so no
                // index can leave v64 .. v(63 + Dq)
                const uint4 p = raw.Q[0][lane];
                const uint32_t pw[3] = {p.x, p.y, p.z};
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const uint32_t b = (pw[k >> 2] >> (8 * (k & 3))) & 0xffu;
                    qv[k >> 2] |= (b <= (uint32_t)Dq ? b : 0u) << (8 * (k & 3));
                }
            } else {
#pragma unroll
                for (int k = 0; k < 12; k++) {   // K = 12 (quick_dma_ok)
                    const int q = quick_code_raw<DT>(raw, lane, k);
                    const uint32_t qb = (q >= 0 && q < Dq) ? (uint32_t)(q + 1) : 0u;
                    qv[k >> 2] |= qb << (8 * (k & 3));
                }
            }
            st.Q[r] = make_uint4(qv[0], qv[1], qv[2], 0u);
        }
        const uint32_t gid_n = idx + 64 < re ? raw.nid[lane] : 0u;
        wave_lds_fence();   // raw read, stage written: raw may be refilled
        if (base + 64 < re) quick_dma12<NQ>(raw, a, gid_n, a.point_list + min(idx + 128, re - 1));
        const int n = __popcll(m);
        // the blend of k_render_fwd_quick_v, unchanged
        for (int j0 = 0; j0 < n; j0 += 2) {
            if (wave_ballot(!done) == 0) break;
            const bool two = j0 + 1 < n;
            const int j1 = two ? j0 + 1 : j0;
            const float4 A0 = st.A[j0], B0 = st.B[j0];
            const float4 A1 = st.A[j1], B1 = st.B[j1];
            // the colours read with the geometry, and the blend below as selects
            // (the same fmaf on the same operands where a pixel takes the
            // candidate): no LDS round trip or exec-mask branch per candidate
            const float4 C0 = st.C[j0], C1 = st.C[j1];
            const float p0 = splat_power(A0.z, A0.w, B0.x, A0.x - pfx, A0.y - pfy);
            const float p1 = splat_power(A1.z, A1.w, B1.x, A1.x - pfx, A1.y - pfy);
            bool ok0 = !done && !(p0 > 0.0f || p0 < B0.z);
            bool ok1 = two && !done && !(p1 > 0.0f || p1 < B1.z);
            if (!wave_any(ok0 || ok1)) continue;
            const f32x2 EX = expf_det2(f32x2{p0, p1});
            const float al0 = fminf(0.99f, B0.y * EX.x);
            const float al1 = fminf(0.99f, B1.y * EX.y);
            ok0 = ok0 && !(al0 < 1.0f / 255.0f);
            ok1 = ok1 && !(al1 < 1.0f / 255.0f);
            float aT0, aT1;
            {
                const float test_T = T * (1.0f - al0);
                const bool term = ok0 && (test_T < 0.0001f);
                done = done || term;
                ok0 = ok0 && !term;
                ok1 = ok1 && !term;
                aT0 = ok0 ? al0 * T : 0.f;
                cr = ok0 ? fmaf(C0.x, aT0, cr) : cr;
                cg = ok0 ? fmaf(C0.y, aT0, cg) : cg;
                cbl = ok0 ? fmaf(C0.z, aT0, cbl) : cbl;
                T = ok0 ? test_T : T;
                last = ok0 ? (uint32_t)__float_as_int(B0.w) : last;
            }
            {
                const float test_T = T * (1.0f - al1);
                const bool term = ok1 && (test_T < 0.0001f);
                done = done || term;
                ok1 = ok1 && !term;
                aT1 = ok1 ? al1 * T : 0.f;
                cr = ok1 ? fmaf(C1.x, aT1, cr) : cr;
                cg = ok1 ? fmaf(C1.y, aT1, cg) : cg;
                cbl = ok1 ? fmaf(C1.z, aT1, cbl) : cbl;
                T = ok1 ? test_T : T;
                last = ok1 ? (uint32_t)__float_as_int(B1.w) : last;
            }
            if (wave_any(ok0)) LSR_QV_UPDATE(aT0, st.Q[j0], st.Wt[j0][0], st.Wt[j0][1], st.Wt[j0][2]);
            if (wave_any(ok1)) LSR_QV_UPDATE(aT1, st.Q[j1], st.Wt[j1][0], st.Wt[j1][1], st.Wt[j1][2]);
        }
        wave_lds_fence();
    }
    // no LDS-DMA may land after the wave (and its LDS) is gone
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const size_t HW = (size_t)c.H * c.W;
    if (inside) {
        const size_t pix = (size_t)pm.py * c.W + pm.px;
        a.final_T[pix] = T;
        a.n_contrib[pix] = last;
        a.out_color[pix] = fmaf(T, c.bg[0], cr);
        a.out_color[HW + pix] = fmaf(T, c.bg[1], cg);
        a.out_color[2 * HW + pix] = fmaf(T, c.bg[2], cbl);
        float* const o = a.out_lang + pix;
        if (a.quick_hwc) {   // Dq == 192 (lsr_api validate)
            float* const row = a.out_lang + pix * 192;
            asm volatile(LSR_QHWC_ALL : : [p] "v"(row) : "memory");
        } else if (Dq == 192 && (uint64_t)HW * 192u * 4u < 0x80000000ull) {
            // all 192 channels straight from v64..v255 by buffer stores, the channel
            // plane's byte offset in an SGPR stepped by HW * 4: two instructions per
            // channel instead of the index-mode read, the M0 save / restore and a
            // 64-bit address per store
            const __amdgpu_buffer_rsrc_t ro =
                __builtin_amdgcn_make_buffer_rsrc(a.out_lang, 0, (int)(HW * 192u * 4u), 0x00020000);
            uint32_t so;
            asm volatile("s_mov_b32 %[so], 0\n\t"
                         LSR_QEPI_ALL
                         : [so] "=&s"(so)
                         : [vo] "v"((uint32_t)pix * 4u), [rs] "s"(ro), [hw4] "s"((uint32_t)HW * 4u)
                         : "memory", "scc");
        } else {
            for (int q = 0; q < Dq; q++) {
                float v;
                uint32_t sv;
                asm volatile(
                    "s_mov_b32 %[sv], m0\n\t"
                    "s_set_gpr_idx_on %[q], gpr_idx(SRC0)\n\t"
                    "s_nop 0\n\t"
                    "v_mov_b32 %[v], v64\n\t"
                    "s_set_gpr_idx_off\n\t"
                    "s_mov_b32 m0, %[sv]"
                    : [v] "=v"(v), [sv] "=&s"(sv)
                    : [q] "s"(q)
                    : "memory");
                o[(size_t)q * HW] = v;
            }
        }
    }
}
#pragma clang diagnostic pop

// the LDS-DMA quick kernel applies: 12 codes per Gaussian (3 levels x top-4), 16-B aligned rows
static bool quick_dma_ok(const RenderArgs& a)
{
    return a.K == 12 && a.Dq <= 192 && ((uintptr_t)a.qw % 16) == 0 && ((uintptr_t)a.qi % 16) == 0 &&
           ((uintptr_t)a.rgb % 4) == 0;
}

// launch_render_fwd's quick arm (a.qw set, at least one tile)
hipError_t launch_render_fwd_quick(const RenderArgs& a, hipStream_t st)
{
    const int T = a.cam.gx * a.cam.gy;
    if (a.quick_hwc && !(quick_dma_ok(a) && a.Dq == 192)) return hipErrorInvalidValue;
    if (a.qidx_dtype == LSR_INDEX_PACKED && !quick_dma_ok(a)) return hipErrorInvalidValue;
    void (*k)(RenderArgs) = k_render_fwd_quick;
    size_t sm = 0;
    if (quick_dma_ok(a)) {
        // DT (quick_nq, quick_code_raw): 0 fp32, 1 int32, 2 int64, 3 packed bytes
        const int dt = a.qidx_dtype == LSR_INDEX_F32 ? 0 : a.qidx_dtype == LSR_INDEX_I32 ? 1
                       : a.qidx_dtype == LSR_INDEX_PACKED ? 3 : 2;
        with_int(std::integer_sequence<int, 0, 1, 2, 3>{}, dt, [&](auto dtc) {
            with_bools([&](auto band) { k = k_render_fwd_quick_d<decltype(dtc)::value, band.value>; }, !a.quick_hwc);
        });
    } else if (a.K <= 12 && a.Dq <= 192) {
        const int np = (a.Dq + 31) / 32;   // accumulator vectors of 32 channels
        with_int(std::integer_sequence<int, 1, 2, 3, 4, 5, 6>{}, np >= 1 && np <= 5 ? np : 6,
                 [&](auto npc) { k = k_render_fwd_quick_v<npc.value>; });
    } else {
        sm = (size_t)a.Dq * 64 * 4 + 64 * 32 + 64 * 12 + (size_t)64 * a.K * 8;
    }
    k<<<T * 4, 64, sm, st>>>(a);
    return hipGetLastError();
}

}  // namespace lsr
