// quick_heat.hip — the viewer's two query maps and their colour stage, fused.
//
// The map kernel (k_quick_heat) is pixel-resident where k_quick_query is
// level-resident: a wave owns a 16-pixel tile and walks its L levels, because
// both quantities need every level of a pixel together.  One (n_pos, H, W) map:
//
//   LSR_HEAT_SUMMED_COSINE (the render server, backend_renderer.py:204-210)
//     f_l = F_l / (|F_l| + eps), s = sum_l f_l, out[q] = s . e_q / (|s| + eps).
//     With a_l = 1 / (|L_l^T w_l| + eps) (the decode's norm factor),
//       s . e_q = sum_l a_l (w_l^T CB_l e_q)          the query plan's projections
//       |s|     = |sum_l C[rows of l]^T (a_l w_l)|    C C^T = the stacked Gram matrix
//     C is the f64 Cholesky factor of the (L K) x (L K) Gram matrix of all
//     codebooks, so |s|^2 is a sum of squares and cannot cancel (f_0 = -f_1
//     leaves the third level's norm, not a difference of O(1) terms).  The
//     levels are stacked in descending order (level L - 1 first): level l then
//     meets only the first 4 (L - l) 16-column blocks of C's rows, and the 64
//     components of group g = L - 1 - l are complete after level l — they are
//     squared and summed at once, so a wave holds 64 (L - 1 - l) partial
//     components per pixel, not 64 L.  4 L + ... + 4 = 2 L (L + 1) blocks: 24 at L = 3.
//   LSR_HEAT_MEAN_RELEVANCY (the prompt demo, demo_prompt.py:122-123)
//     out[q] = (sum_l rel_l[q]) / L in level order, rel_l the statements of
//     k_quick_query.
//
// The colour stage (k_heat_frame) is the servers' host tail on the device:
// per-plane gate, curve, 256-entry table, optional blend with the RGB render,
// uint8 pixel-major.  Every operation is fp32 and rounded on its own (the
// build has -ffp-contract=off), so a numpy float32 restatement has its bytes.
#include "quick_common.h"

namespace lsr {

#ifndef LSR_HEAT_PB
// 16-pixel blocks per tile.  The stacked product's partial components cost 16 (L - 1) VGPRs per block
// on top of the tile's weights, fragments and numerators: at L = 3 one block compiles to 164-176 VGPRs,
// two blocks to 256 with 64-71 spilled, and the workgroup's 8 waves need 2 waves per SIMD (256 each)
#define LSR_HEAT_PB 1
#endif
constexpr int HPB = LSR_HEAT_PB, HTILE = 16 * HPB;
constexpr int HEAT_MAXL = 3;
constexpr int HEAT_LDS_BLOCKS = 40;   // 4-KB fragment blocks a workgroup may keep in LDS (160 KB)

// Lower triangle of the stacked Gram matrix in f64, levels in descending order:
// stacked row i = 64 p + k is code k of level L - 1 - p.  One 16 x 16 tile per
// workgroup (tiles above the diagonal are skipped), staged 128 dims at a time.
__global__ void __launch_bounds__(256) k_heat_gram(const float* __restrict__ cb, int L, int K, int Df,
                                                   double* __restrict__ G)
{
    __shared__ float sa[16][129], sb[16][129];
    const int n = L * K, nt = n / 16;
    const int ti = (int)blockIdx.x / nt, tj = (int)blockIdx.x % nt;
    if (tj > ti) return;
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    auto row = [&](int i) { return cb + ((size_t)(L - 1 - i / K) * K + i % K) * Df; };
    double v = 0.0;
    for (int d0 = 0; d0 < Df; d0 += 128) {
        __syncthreads();
        for (int e = threadIdx.x; e < 16 * 128; e += 256) {
            const int rr = e >> 7, dd = e & 127;
            const bool ok = d0 + dd < Df;
            sa[rr][dd] = ok ? row(16 * ti + rr)[d0 + dd] : 0.f;
            sb[rr][dd] = ok ? row(16 * tj + rr)[d0 + dd] : 0.f;
        }
        __syncthreads();
        for (int dd = 0; dd < 128; dd++) v += (double)sa[r][dd] * (double)sb[c][dd];
    }
    G[(size_t)(16 * ti + r) * n + 16 * tj + c] = v;
}

// C C^T = G for the stacked matrix (n = L K <= 192), f64, the lower triangle
// packed in LDS, right-looking with the pivot rule of k_codebook_chol: a pivot
// at or below 1e-12 of the largest diagonal entry leaves its column zero
// (identical or negated levels make G singular).  Output as L "codebooks" of
// K rows and n columns — Cf[l][k][c] = C[64 (L - 1 - l) + k][c], zeros above
// the diagonal — which is the form k_codebook_frag packs.
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }

__global__ void __launch_bounds__(1024) k_heat_chol(const double* __restrict__ G, int L, int K, float* __restrict__ Cf)
{
    extern __shared__ double A[];   // n (n + 1) / 2
    __shared__ double s_tol;
    const int n = L * K, t = threadIdx.x;
    for (int e = t; e < n * n; e += 1024) {
        const int i = e / n, j = e % n;
        if (j <= i) A[tri(i, j)] = G[e];
    }
    __syncthreads();
    if (t == 0) {
        double mx = 0.0;
        for (int j = 0; j < n; j++) mx = fmax(mx, A[tri(j, j)]);
        s_tol = 1e-12 * mx;
    }
    __syncthreads();
    const double tol = s_tol;
    for (int j = 0; j < n; j++) {
        const double d = A[tri(j, j)];
        const double piv = d > tol ? sqrt(d) : 0.0;
        __syncthreads();   // every thread has read the pivot
        if (t == j) A[tri(j, j)] = piv;
        if (t > j && t < n) A[tri(t, j)] = piv > 0.0 ? A[tri(t, j)] / piv : 0.0;
        __syncthreads();
        const int m = n - 1 - j;
        for (int e = t; e < m * m; e += 1024) {
            const int i = j + 1 + e / m, k = j + 1 + e % m;
            if (k <= i) A[tri(i, k)] -= A[tri(i, j)] * A[tri(k, j)];
        }
        __syncthreads();
    }
    for (int e = t; e < n * n; e += 1024) {
        const int i = e / n, c = e % n;
        const int l = L - 1 - i / K, k = i % K;
        Cf[((size_t)l * K + k) * n + c] = c <= i ? (float)A[tri(i, c)] : 0.f;
    }
}

// the plan's fragment tables as the kernel reads them
struct HeatFrags {
    const uint4* pfrag;      // [l][cb] projections
    const float* pscales;
    const uint4* nfrag;      // [l][mb] per-level norm factor
    const float* nscales;
    const uint4* sfrag;      // [l][jb < 4 L] stacked factor (blocks jb >= 4 (L - l) are zero)
    const float* sscales;
};

// first LDS block of level l's stacked-factor blocks: sum over l' < l of 4 (L - l')
__host__ __device__ constexpr int heat_soff(int L, int l) { return 4 * l * L - 2 * l * (l - 1); }

template <int L, bool MEAN, bool SLDS, bool HWC>
__global__ void __launch_bounds__(64 * LSR_DEC2_WAVES, 1)
    k_quick_heat(const float* __restrict__ wmap, int W, int H, HeatFrags p, float* __restrict__ out, float eps,
                 float scale, int n_pos, int n_neg, int NCB, int vec)
{
    extern __shared__ uint4 sfr[];   // [l][cb] projection, [l][mb] norm factor, then each level's stacked-factor blocks
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
    const int NO = L * NCB, SO = NO + 4 * L;
    {
        for (int i = threadIdx.x; i < NO * 256; i += 64 * LSR_DEC2_WAVES) sfr[i] = p.pfrag[i];
        for (int i = threadIdx.x; i < 4 * L * 256; i += 64 * LSR_DEC2_WAVES) sfr[NO * 256 + i] = p.nfrag[i];
        if constexpr (!MEAN && SLDS) {
#pragma unroll
            for (int l = 0; l < L; l++) {
                const uint4* src = p.sfrag + (size_t)l * 4 * L * 256;
                uint4* dst = sfr + (size_t)(SO + heat_soff(L, l)) * 256;
                for (int i = threadIdx.x; i < 4 * (L - l) * 256; i += 64 * LSR_DEC2_WAVES) dst[i] = src[i];
            }
        }
    }
    __syncthreads();
    const size_t HW = (size_t)W * H;
    const int nbx = (W + HTILE - 1) / HTILE;
    const int ntile = nbx * H;
    const int stride = (int)gridDim.x * LSR_DEC2_WAVES;
    const int lk = L * 64;
    const int nbn = (n_neg + 15) >> 4;   // blocks holding negatives
    const int cb0 = n_neg >> 4;          // the first block holding a positive
    float raw[HPB][2][8];
    int t = (int)blockIdx.x * LSR_DEC2_WAVES + w;
    dec_load_tile<HWC, HPB>(raw, wmap, t, ntile, nbx, W, HW, 0, lk, li, lg);
    for (; t < ntile; t += stride) {
        const int bx = (t % nbx) * HTILE, y = t / nbx;
        // SUMMED: num[cb] = s . e of block cb's columns, ssq = this lane's share of |s|^2, Yp = the
        // incomplete component groups.  MEAN: num[cbi] = sum of the relevancies of block cb0 + cbi
        float num[4][HPB][4], ssq[HPB][4], Yp[L > 1 ? L - 1 : 1][4][HPB][4];
#pragma unroll
        for (int pb = 0; pb < HPB; pb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                ssq[pb][r] = 0.f;
#pragma unroll
                for (int cb = 0; cb < 4; cb++) num[cb][pb][r] = 0.f;
#pragma unroll
                for (int g = 0; g < L - 1; g++)
#pragma unroll
                    for (int mb = 0; mb < 4; mb++) Yp[g][mb][pb][r] = 0.f;
            }
        // (the level loop is rolled: register arrays are indexed by unrolled inner loops only, and
        // each block product is fenced so its fragment loads are not hoisted over the ones before)
#pragma unroll 1
        for (int l = 0; l < L; l++) {
            float psc[HPB];
            h8 Wh[HPB][2], Wl[HPB][2];
            dec_scale_split(raw, psc, Wh, Wl);
            // the next level's weights (or the next tile's first level) in flight during this level's products
            const bool last = l + 1 == L;
            dec_load_tile<HWC, HPB>(raw, wmap, last ? t + stride : t, ntile, nbx, W, HW, last ? 0 : l + 1, lk, li, lg);
            // |F_l|^2 = |L_l^T w|^2 (as k_quick_query)
            float sq[HPB][4];
#pragma unroll
            for (int pb = 0; pb < HPB; pb++)
#pragma unroll
                for (int r = 0; r < 4; r++) sq[pb][r] = 0.f;
#pragma unroll 1
            for (int mb = 0; mb < 4; mb++) {
                const uint4* f = sfr + (size_t)(NO + 4 * l + mb) * 256 + lane * 2;
                const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
                const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
                for (int pb = 0; pb < HPB; pb++) {
                    f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                    LSR_DEC_MFMA6(acc, pb);
#pragma unroll
                    for (int r = 0; r < 4; r++) sq[pb][r] = fmaf(acc[r], acc[r], sq[pb][r]);
                }
            }
            // both products run on the scaled weights w / osc, so eps becomes eps / osc (quick_query.hip)
            const float sc = p.pscales[l];
            const float ns2 = p.nscales[l] * p.nscales[l];
            float den[HPB][4];
#pragma unroll
            for (int pb = 0; pb < HPB; pb++) {
                const float ipsc = 1.f / psc[pb];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float iosc = __shfl(ipsc, 4 * lg + r, 64);
                    den[pb][r] = sqrtf(fmaxf(row16_sum(sq[pb][r]) * ns2, 0.f)) + eps * iosc;
                }
            }
            if constexpr (MEAN) {
                float mul[HPB][4], mneg[HPB][4];
#pragma unroll
                for (int pb = 0; pb < HPB; pb++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        mul[pb][r] = sc / den[pb][r];
                        mneg[pb][r] = -INFINITY;
                    }
                f32x4q v[HPB];
                auto sims = [&](int cb) {
                    const uint4* f = sfr + (size_t)(l * NCB + cb) * 256 + lane * 2;
                    const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
                    const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
                    for (int pb = 0; pb < HPB; pb++) {
                        f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                        LSR_DEC_MFMA6(acc, pb);
#pragma unroll
                        for (int r = 0; r < 4; r++) v[pb][r] = acc[r] * mul[pb][r];
                    }
                };
#pragma unroll 1
                for (int cb = 0; cb < nbn; cb++) {
                    sims(cb);
                    const bool isneg = 16 * cb + li < n_neg;
#pragma unroll
                    for (int pb = 0; pb < HPB; pb++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            mneg[pb][r] = fmaxf(mneg[pb][r], row16_max(isneg ? v[pb][r] : -INFINITY));
                }
#pragma unroll
                for (int cbi = 0; cbi < 4; cbi++) {
                    if (cb0 + cbi >= NCB) break;
                    sims(cb0 + cbi);
#pragma unroll
                    for (int pb = 0; pb < HPB; pb++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            num[cbi][pb][r] += __builtin_amdgcn_rcpf(1.f + expf(scale * (mneg[pb][r] - v[pb][r])));
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                // a_l with each table's power-of-two scale folded in
                const float ss = p.sscales[l];
                float mulp[HPB][4], muls[HPB][4];
#pragma unroll
                for (int pb = 0; pb < HPB; pb++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float a = 1.f / den[pb][r];
                        mulp[pb][r] = sc * a;
                        muls[pb][r] = ss * a;
                    }
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    if (cb >= NCB) break;
                    const uint4* f = sfr + (size_t)(l * NCB + cb) * 256 + lane * 2;
                    const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
                    const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
                    for (int pb = 0; pb < HPB; pb++) {
                        f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                        LSR_DEC_MFMA6(acc, pb);
#pragma unroll
                        for (int r = 0; r < 4; r++) num[cb][pb][r] += acc[r] * mulp[pb][r];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                // Y += C[rows of l]^T (a_l w_l): groups 0 .. L - 1 - l, the last of them complete
                const uint4* sbase;
                if constexpr (SLDS) sbase = sfr + (size_t)(SO + heat_soff(L, l)) * 256 + lane * 2;
                else sbase = p.sfrag + (size_t)(l * 4 * L) * 256 + lane * 2;
#pragma unroll
                for (int g = 0; g < L; g++) {
                    if (g >= L - l) break;
                    const bool complete = g == L - 1 - l;
#pragma unroll
                    for (int mb = 0; mb < 4; mb++) {
                        const uint4* f = sbase + (size_t)(4 * g + mb) * 256;
                        const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
                        const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
                        for (int pb = 0; pb < HPB; pb++) {
                            f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                            LSR_DEC_MFMA6(acc, pb);
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                float yv = acc[r] * muls[pb][r];
                                if (g < L - 1) yv += Yp[g < L - 1 ? g : 0][mb][pb][r];
                                if (complete) ssq[pb][r] = fmaf(yv, yv, ssq[pb][r]);
                                else if (g < L - 1) Yp[g < L - 1 ? g : 0][mb][pb][r] = yv;
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
        // lane (li, lg) holds column li of each block for pixels 16 pb + 4 lg + r
        float sden[HPB][4];   // |s| + eps
#pragma unroll
        for (int pb = 0; pb < HPB; pb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if constexpr (MEAN) sden[pb][r] = 1.f;
                else sden[pb][r] = sqrtf(row16_sum(ssq[pb][r])) + eps;
            }
#pragma unroll
        for (int cbi = 0; cbi < 4; cbi++) {
            const int cb = MEAN ? cb0 + cbi : cbi;
            if (cb >= NCB) break;
            const int q = 16 * cb + li - n_neg;
            const bool isq = q >= 0 && q < n_pos;   // else a negative's or a padding column's lane
            float* const orow = out + (size_t)(isq ? q : 0) * HW + (size_t)y * W;
#pragma unroll
            for (int pb = 0; pb < HPB; pb++) {
                if (!isq) continue;
                float o4[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if constexpr (MEAN) o4[r] = num[cbi][pb][r] / (float)L;
                    else o4[r] = num[cbi][pb][r] / sden[pb][r];
                }
                const int xo = bx + 16 * pb + 4 * lg;
                float* o = orow + xo;
                if (vec && xo + 3 < W) {
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

// The heat plan: the query plan's pieces (projection fragments, the per-level
// norm factor chain, the f32 projection) and the stacked factor's chain: the
// f64 Gram matrix, the factor as L codebooks of L K columns, its fragments
// and scales.  A buffer of its own: the query plan's size is part of the ABI.
struct HeatPlan {
    uint4* pfrag;
    float* pscales;
    float* G;
    float* Lf;
    uint4* nfrag;
    float* nscales;
    float* P;
    double* G64;
    float* Cf;
    uint4* sfrag;
    float* sscales;
    size_t bytes;
};

static HeatPlan heat_plan_layout(const void* ws, int L, int K, int ncp)
{
    auto up = [](size_t n) { return (n + 255) / 256 * 256; };
    const uintptr_t p = (uintptr_t)ws;   // (nullptr: only .bytes is used)
    const size_t n = (size_t)L * K;
    HeatPlan h;
    size_t o = 0;
    h.pfrag = (uint4*)(p + o);    o += (size_t)L * (ncp / 16) * 4096;
    h.pscales = (float*)(p + o);  o += up((size_t)L * 4);
    h.G = (float*)(p + o);        o += (size_t)L * K * K * 4;
    h.Lf = (float*)(p + o);       o += (size_t)L * K * K * 4;
    h.nfrag = (uint4*)(p + o);    o += (size_t)L * 4 * 4096;
    h.nscales = (float*)(p + o);  o += up((size_t)L * 4);
    h.P = (float*)(p + o);        o += up((size_t)L * K * ncp * 4);
    h.G64 = (double*)(p + o);     o += up(n * n * 8);
    h.Cf = (float*)(p + o);       o += up((size_t)L * K * n * 4);
    h.sfrag = (uint4*)(p + o);    o += (size_t)L * (n / 16) * 4096;
    h.sscales = (float*)(p + o);  o += up((size_t)L * 4);
    h.bytes = o;
    return h;
}

static int heat_ncp(int n_pos, int n_neg) { return (n_pos + n_neg + 15) / 16 * 16; }

size_t quick_heat_plan_bytes(int L, int K, int n_pos, int n_neg)
{
    return heat_plan_layout(nullptr, L, K, heat_ncp(n_pos, n_neg)).bytes;
}

hipError_t launch_quick_heat_prepare(const float* cb, const float* pos, const float* neg, int L, int K, int Df,
                                     int n_pos, int n_neg, void* ws, hipStream_t st)
{
    if (L == 0) return hipSuccess;
    const int ncp = heat_ncp(n_pos, n_neg);
    const HeatPlan h = heat_plan_layout(ws, L, K, ncp);
    launch_query_project(cb, pos, neg, L, K, Df, n_pos, n_neg, ncp, h.P, st);
    launch_codebook_frag(h.P, L, K, ncp, h.pfrag, h.pscales, st);
    norm_factor_prepare(cb, L, K, Df, h.G, h.Lf, h.nfrag, h.nscales, true, st);
    const int n = L * K, nt = n / 16;
    k_heat_gram<<<(unsigned)(nt * nt), 256, 0, st>>>(cb, L, K, Df, h.G64);
    const size_t lds = (size_t)n * (n + 1) / 2 * sizeof(double);
    (void)hipFuncSetAttribute((const void*)k_heat_chol, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    k_heat_chol<<<1, 1024, lds, st>>>(h.G64, L, K, h.Cf);
    launch_codebook_frag(h.Cf, L, K, n, h.sfrag, h.sscales, st);
    return hipGetLastError();
}

template <int L>
static void heat_launch(const float* wmap, const HeatPlan& h, bool mean, bool hwc, int n_pos, int n_neg, int H, int W,
                        float scale, float eps, float* out, hipStream_t st)
{
    const int NCB = heat_ncp(n_pos, n_neg) / 16;
    const int resident = L * NCB + 4 * L;
    // the stacked factor's blocks stay in LDS when they fit beside the projections and the norm factors
    // (L = 3: up to 16 columns), else the product reads them from L2
    const bool slds = mean || resident + 2 * L * (L + 1) <= HEAT_LDS_BLOCKS;
    const size_t lds = (size_t)(resident + (!mean && slds ? 2 * L * (L + 1) : 0)) * 256 * sizeof(uint4);
    const int ntile = (W + HTILE - 1) / HTILE * H;
    const int need = (ntile + LSR_DEC2_WAVES - 1) / LSR_DEC2_WAVES;
    const int nwg = need < cu_count() ? need : cu_count();
    const int vec = (W % 4) == 0 && ((uintptr_t)out % 16) == 0;
    const HeatFrags f = {h.pfrag, h.pscales, h.nfrag, h.nscales, h.sfrag, h.sscales};
    with_bools([&](auto meanc, auto sldsc, auto hwcc) {
        // (mean relevancy has no stacked product; only L = 3 can overflow the LDS)
        if constexpr ((meanc.value || L < 3) && !sldsc.value) {
            return;
        } else {
            auto kern = k_quick_heat<L, meanc.value, sldsc.value, hwcc.value>;
            (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            kern<<<(unsigned)nwg, 64 * LSR_DEC2_WAVES, lds, st>>>(wmap, W, H, f, out, eps, scale, n_pos, n_neg, NCB,
                                                                vec);
        }
    }, mean, slds, hwc);
}

hipError_t launch_quick_heat_run(const float* wmap, bool hwc, const void* ws, int L, int K, int n_pos, int n_neg,
                                 int H, int W, bool mean, float scale, float eps, float* out, hipStream_t st)
{
    if (L == 0 || H == 0 || W == 0) return hipSuccess;
    if (L > HEAT_MAXL) return hipErrorInvalidValue;
    const HeatPlan h = heat_plan_layout(ws, L, K, heat_ncp(n_pos, n_neg));
    if (L == 1) heat_launch<1>(wmap, h, mean, hwc, n_pos, n_neg, H, W, scale, eps, out, st);
    else if (L == 2) heat_launch<2>(wmap, h, mean, hwc, n_pos, n_neg, H, W, scale, eps, out, st);
    else heat_launch<3>(wmap, h, mean, hwc, n_pos, n_neg, H, W, scale, eps, out, st);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Colour, blend, pack: maps (planes, H, W) fp32 with per-plane stats
// {min, max, .} (lsr_query_smooth's rows) -> out (planes, H, W, 3) uint8.
// A thread takes 4 consecutive pixels of a plane: 12 output bytes.
constexpr int HF_THREADS = 256;

template <bool POWER4, bool RGB>
__global__ void __launch_bounds__(HF_THREADS) k_heat_frame(const float* __restrict__ maps,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ rgb,
                                                           const uint8_t* __restrict__ lut, int HW, float threshold,
                                                           float min_range, float alpha, uint8_t* __restrict__ out,
                                                           int vec)
{
    __shared__ uint8_t s_lut[768];
    for (int i = threadIdx.x; i < 768; i += HF_THREADS) s_lut[i] = lut[i];
    __syncthreads();
    const int plane = blockIdx.y;
    const float mn = stats[(size_t)plane * 3 + 0], mx = stats[(size_t)plane * 3 + 1];
    const float range = mx - mn;
    const bool gate = mx < threshold || range < min_range;
    const float den = range + (POWER4 ? 1e-8f : 1e-9f);
    const float ialpha = 1.f - alpha;
    const float* src = maps + (size_t)plane * HW;
    uint8_t* dst = out + (size_t)plane * HW * 3;
    const int i0 = ((int)blockIdx.x * HF_THREADS + (int)threadIdx.x) * 4;
    if (i0 >= HW) return;
    const bool full = vec && i0 + 3 < HW;
    float x[4];
    if (full) {
        const float4 v = *reinterpret_cast<const float4*>(src + i0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = i0 + k < HW ? src[i0 + k] : 0.f;
    }
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = 0.f;
        if (!gate) {
            const float tt = (x[k] - mn) / den;
            if constexpr (POWER4) v = (tt * tt) * (tt * tt);
            else v = fminf(fmaxf(tt * 2.f - 1.f, 0.f), 1.f);
        }
        // truncation as .astype(uint8); a non-finite v still indexes inside the table
        const float s255 = v * 255.f;
        int idx = s255 >= 0.f ? (s255 <= 255.f ? (int)s255 : 255) : 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint8_t heat = s_lut[idx * 3 + c];
            if constexpr (RGB) {
                const float rv = i0 + k < HW ? rgb[(size_t)c * HW + i0 + k] : 0.f;
                float col = rv * ialpha + ((float)heat / 255.f) * alpha;
                col = fminf(fmaxf(col, 0.f), 1.f);
                b[3 * k + c] = (uint8_t)(int)(col * 255.f);
            } else {
                b[3 * k + c] = heat;
            }
        }
    }
    if (full) {
        uint32_t* o = reinterpret_cast<uint32_t*>(dst + (size_t)i0 * 3);
#pragma unroll
        for (int d = 0; d < 3; d++)
            o[d] = (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) |
                   ((uint32_t)b[4 * d + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i0 + k < HW)
#pragma unroll
                for (int c = 0; c < 3; c++) dst[(size_t)(i0 + k) * 3 + c] = b[3 * k + c];
    }
}

bool heat_frame_shape_ok(int planes, int H, int W)
{
    return planes >= 0 && H >= 0 && W >= 0 && planes <= 65535 && (int64_t)H * W <= (int64_t)0x7fffffff - 4 * HF_THREADS;
}

hipError_t launch_heat_frame(const float* maps, const float* stats, const float* rgb, const uint8_t* lut, int planes,
                             int H, int W, bool power4, float threshold, float min_range, float alpha, uint8_t* out,
                             hipStream_t st)
{
    if (planes == 0 || H == 0 || W == 0) return hipSuccess;
    const int HW = H * W;
    // 16-B map reads and 4-B packed stores: every plane must start aligned
    const int vec = (HW % 4) == 0 && ((uintptr_t)maps % 16) == 0 && ((uintptr_t)out % 4) == 0;
    const dim3 grid((unsigned)((HW + 4 * HF_THREADS - 1) / (4 * HF_THREADS)), (unsigned)planes);
    with_bools([&](auto p4, auto hasrgb) {
        k_heat_frame<p4.value, hasrgb.value><<<grid, HF_THREADS, 0, st>>>(maps, stats, rgb, lut, HW, threshold,
                                                                         min_range, alpha, out, vec);
    }, power4, rgb != nullptr);
    return hipGetLastError();
}

}  // namespace lsr
