// quick_query.hip — fused text-query relevancy of the quick language map
// (replaces, after the decode of quick_decode.hip, the reference's
// OpenCLIPNetwork.get_max_across_quick, eval/openclip_encoder.py:114-139).  The
// (L, Df, H, W) feature map never exists: with pixel weights w (K), codebook
// CB_l (K x Df) and a unit text embedding e,
//   f . e = w^T (CB_l e)            one column of P_l = CB_l E^T (K x (N_neg + Q)), per query set
//   |f|   = |L_l^T w|               the decode's Cholesky norm factor
//   sim   = f . e / (|f| + eps)
// and the reference's softmax over (10 sim_pos, 10 sim_neg_j) followed by the
// min over j is 1 / (1 + exp(scale (max_j sim_neg_j - sim_pos))) for scale >= 0.
// Per pixel and level: one K x (64 + 16 NCB) product on the decode's A
// fragments (quick_common.h), 768 B read, 4 Q B written.
#include "quick_common.h"

namespace lsr {

// P[l][k][c] = sum_d CB[l][k][d] E[c][d], the 512-term dot in f64; columns: the
// n_neg negatives, then the n_pos positives, then zeros up to ncp (a multiple of 16).
__global__ void __launch_bounds__(256) k_query_project(const float* __restrict__ cb, const float* __restrict__ pos,
                                                       const float* __restrict__ neg, int K, int Df, int n_pos,
                                                       int n_neg, int ncp, float* __restrict__ P)
{
    const int l = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= K * ncp) return;
    const int k = idx / ncp, c = idx % ncp;
    double s = 0.0;
    if (c < n_neg + n_pos) {
        const float* a = cb + ((size_t)l * K + k) * Df;
        const float* e = c < n_neg ? neg + (size_t)c * Df : pos + (size_t)(c - n_neg) * Df;
        for (int d = 0; d < Df; d++) s += (double)a[d] * (double)e[d];
    }
    P[(size_t)l * K * ncp + idx] = (float)s;
}

// Level-resident like k_quick_decode_l: the level's NCB projection blocks and the
// 4 norm-factor blocks (4 KB each) stay in LDS, a wave takes 64-pixel tiles with
// the next tile's weights in flight.  A product block leaves its 16 columns
// across a row's 16 lanes (lane li = column, registers = pixels 4 lg + r), so
// the maximum over the negative columns is a masked 16-lane reduction; blocks
// 0 .. (n_neg - 1) / 16 hold negatives and are reduced first, the last of them
// (which may also hold positives) stays in registers for the output pass.
// REL: out (L, n_pos, H, W) = relevancy; else the cosine similarities of the positives.
template <bool REL, bool VEC, bool HWC>
__global__ void __launch_bounds__(64 * LSR_DEC2_WAVES, 1)
    k_quick_query(const float* __restrict__ wmap, int W, int H, const uint4* __restrict__ pfrag,
                  const float* __restrict__ pscales, const uint4* __restrict__ nfrag,
                  const float* __restrict__ nscales, float* __restrict__ out, float eps, float scale, int nwg, int lk,
                  int n_pos, int n_neg, int NCB)
{
    extern __shared__ uint4 sfr[];   // [cb][s][lane][hi, lo] projection, then 4 blocks of the norm factor
    const int l = (int)blockIdx.x / nwg, wi = (int)blockIdx.x % nwg;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
    {
        const uint4* src = pfrag + (size_t)l * NCB * 256;
        for (int i = threadIdx.x; i < NCB * 256; i += 64 * LSR_DEC2_WAVES) sfr[i] = src[i];
        const uint4* ns = nfrag + (size_t)l * 4 * 256;
        for (int i = threadIdx.x; i < 4 * 256; i += 64 * LSR_DEC2_WAVES) sfr[NCB * 256 + i] = ns[i];
    }
    __syncthreads();
    const float sc = pscales[l];
    const float ns2 = nscales[l] * nscales[l];
    const size_t HW = (size_t)W * H;
    const int nbx = (W + 63) / 64;
    const int ntile = nbx * H;
    const int stride = nwg * LSR_DEC2_WAVES;
    const int nbn = (n_neg + 15) >> 4;   // blocks holding negatives
    const int cb0 = n_neg >> 4;          // the first block holding a positive
    float raw[4][2][8];
    int t = wi * LSR_DEC2_WAVES + w;
    dec_load_tile<HWC>(raw, wmap, t, ntile, nbx, W, HW, l, lk, li, lg);
    for (; t < ntile; t += stride) {
        const int bx = (t % nbx) * 64, y = t / nbx;
        float psc[4];
        h8 Wh[4][2], Wl[4][2];
        dec_scale_split(raw, psc, Wh, Wl);   // sim is invariant to the scale but for eps (below)
        dec_load_tile<HWC>(raw, wmap, t + stride, ntile, nbx, W, HW, l, lk, li, lg);
        // Y^T = W^T L: lane (k = 16 mb + li, lg) gets Y[k] of pixels 4 lg + r; |f|^2 = sum_k Y[k]^2
        float sq[4][4];
#pragma unroll
        for (int pb = 0; pb < 4; pb++)
#pragma unroll
            for (int r = 0; r < 4; r++) sq[pb][r] = 0.f;
#pragma unroll 1
        for (int mb = 0; mb < 4; mb++) {
            const uint4* f = sfr + (size_t)(NCB + mb) * 256 + lane * 2;
            const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
            const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                LSR_DEC_MFMA6(acc, pb);
#pragma unroll
                for (int r = 0; r < 4; r++) sq[pb][r] = fmaf(acc[r], acc[r], sq[pb][r]);
            }
        }
        // sim = (w . P) / (|f| + eps) with both products taken on the scaled weights
        // w / osc: eps becomes eps / osc, exactly as in the decode (osc is a power of
        // two within the normal range, so the product with 1 / osc has the quotient's bits)
        float mul[4][4];
#pragma unroll
        for (int pb = 0; pb < 4; pb++) {
            const float ipsc = 1.f / psc[pb];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float iosc = __shfl(ipsc, 4 * lg + r, 64);
                mul[pb][r] = sc / (sqrtf(fmaxf(row16_sum(sq[pb][r]) * ns2, 0.f)) + eps * iosc);
            }
        }
        f32x4q v[4];
        auto sims = [&](int cb) {
            const uint4* f = sfr + (size_t)cb * 256 + lane * 2;
            const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
            const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                LSR_DEC_MFMA6(acc, pb);
#pragma unroll
                for (int r = 0; r < 4; r++) v[pb][r] = acc[r] * mul[pb][r];
            }
        };
        float mneg[4][4];
        if constexpr (REL) {
#pragma unroll
            for (int pb = 0; pb < 4; pb++)
#pragma unroll
                for (int r = 0; r < 4; r++) mneg[pb][r] = -INFINITY;
#pragma unroll 1
            for (int cb = 0; cb < nbn; cb++) {
                sims(cb);
                const bool isneg = 16 * cb + li < n_neg;
#pragma unroll
                for (int pb = 0; pb < 4; pb++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        mneg[pb][r] = fmaxf(mneg[pb][r], row16_max(isneg ? v[pb][r] : -INFINITY));
            }
        }
#pragma unroll 1
        for (int cb = cb0; cb < NCB; cb++) {
            if (!REL || cb >= nbn) sims(cb);   // block nbn - 1 is still in v
            const int q = 16 * cb + li - n_neg;
            const bool isq = q >= 0 && q < n_pos;   // else a negative's or a padding column's lane
            float* const orow = out + ((size_t)l * n_pos + (isq ? q : 0)) * HW + (size_t)y * W;
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                if (!isq) continue;
                float o4[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    // (v_rcp_f32: 1 ulp, and exact for the all-zero pixel's 1 / 2)
                    if constexpr (REL) o4[r] = __builtin_amdgcn_rcpf(1.f + expf(scale * (mneg[pb][r] - v[pb][r])));
                    else o4[r] = v[pb][r];
                }
                const int xo = bx + 16 * pb + 4 * lg;
                float* o = orow + xo;
                if (VEC && xo + 3 < W) {
                    *reinterpret_cast<float4*>(o) = make_float4(o4[0], o4[1], o4[2], o4[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (xo + r < W) o[r] = o4[r];
                }
            }
        }
    }
}

// The query plan: projection fragments (L x NCB x 4 KB) + scales, the norm
// factor chain of the decode plan (Gram matrices, Cholesky factors, the
// factors' fragments + scales), and the f32 projection the fragments are packed from.
struct QueryPlan {
    uint4* pfrag;
    float* pscales;
    float* G;
    float* Lf;
    uint4* nfrag;
    float* nscales;
    float* P;
    size_t bytes;
};

static QueryPlan query_plan_layout(void* ws, int L, int K, int ncp)
{
    auto up = [](size_t n) { return (n + 255) / 256 * 256; };
    const uintptr_t p = (uintptr_t)ws;   // (nullptr: only .bytes is used)
    QueryPlan q;
    size_t o = 0;
    q.pfrag = (uint4*)(p + o);   o += (size_t)L * (ncp / 16) * 4096;
    q.pscales = (float*)(p + o); o += up((size_t)L * 4);
    q.G = (float*)(p + o);       o += (size_t)L * K * K * 4;
    q.Lf = (float*)(p + o);      o += (size_t)L * K * K * 4;
    q.nfrag = (uint4*)(p + o);   o += (size_t)L * 4 * 4096;
    q.nscales = (float*)(p + o); o += up((size_t)L * 4);
    q.P = (float*)(p + o);       o += up((size_t)L * K * ncp * 4);
    q.bytes = o;
    return q;
}

void launch_query_project(const float* cb, const float* pos, const float* neg, int L, int K, int Df, int n_pos,
                          int n_neg, int ncp, float* P, hipStream_t st)
{
    k_query_project<<<dim3((unsigned)((K * ncp + 255) / 256), (unsigned)L), 256, 0, st>>>(cb, pos, neg, K, Df, n_pos,
                                                                                        n_neg, ncp, P);
}

static int query_ncp(int n_pos, int n_neg) { return (n_pos + n_neg + 15) / 16 * 16; }

size_t quick_query_plan_bytes(int L, int K, int n_pos, int n_neg)
{
    return query_plan_layout(nullptr, L, K, query_ncp(n_pos, n_neg)).bytes;
}

hipError_t launch_quick_query_prepare(const float* cb, const float* pos, const float* neg, int L, int K, int Df,
                                      int n_pos, int n_neg, void* ws, hipStream_t st)
{
    if (L == 0) return hipSuccess;
    const int ncp = query_ncp(n_pos, n_neg);
    const QueryPlan q = query_plan_layout(ws, L, K, ncp);
    launch_query_project(cb, pos, neg, L, K, Df, n_pos, n_neg, ncp, q.P, st);
    launch_codebook_frag(q.P, L, K, ncp, q.pfrag, q.pscales, st);
    norm_factor_prepare(cb, L, K, Df, q.G, q.Lf, q.nfrag, q.nscales, true, st);
    return hipGetLastError();
}

hipError_t launch_quick_query_run(const float* wmap, bool hwc, const void* ws, int L, int K, int n_pos, int n_neg,
                                  int H, int W, bool relevancy, float scale, float eps, float* out, hipStream_t st)
{
    if (L == 0 || H == 0 || W == 0) return hipSuccess;
    const int ncp = query_ncp(n_pos, n_neg);
    const QueryPlan q = query_plan_layout(const_cast<void*>(ws), L, K, ncp);
    const bool vec = (W % 4) == 0 && ((uintptr_t)out % 16) == 0;
    const int ncu = cu_count();
    const int nwg = ncu / L > 0 ? ncu / L : 1;
    const int NCB = ncp / 16;
    const size_t lds = (size_t)(NCB + 4) * 256 * sizeof(uint4);
    with_bools([&](auto rel, auto vecc, auto hwcc) {
        k_quick_query<rel.value, vecc.value, hwcc.value><<<(unsigned)(nwg * L), 64 * LSR_DEC2_WAVES, lds, st>>>(
            wmap, W, H, q.pfrag, q.pscales, q.nfrag, q.nscales, out, eps, scale, nwg, L * K, n_pos, n_neg, NCB);
    }, relevancy, vec, hwc);
    return hipGetLastError();
}

}  // namespace lsr
