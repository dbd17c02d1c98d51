// quick_semantic.hip — fused open-vocabulary label maps of the quick language map
// (replaces, after the decode of quick_decode.hip, the reference's
// OpenCLIPNetwork.get_semantic_map, eval/openclip_encoder.py:82-94), the level
// merge and the confusion counts of an evaluation against annotated labels.
// As in quick_query.hip the (L, Df, H, W) feature map never exists: with pixel
// weights w (K), codebook CB_l (K x Df) and the embeddings E = [labels; negatives],
//   f . e_j = w^T (CB_l e_j)        column j of P_l = CB_l E^T (K x (C + N))
//   |f|     = |L_l^T w|             the decode's Cholesky norm factor
//   s_j     = f . e_j / (|f| + eps)
//   label   = argmax_j s_j (lowest j on ties), -1 when j >= C
//   score   = softmax(scale s)[argmax] = 1 / sum_j exp(scale (s_j - s_max))
// Columns are in the reference's order (labels, then negatives), so the lowest
// column of a tie is torch.argmax's.  The arg-max is taken on the raw products
// w^T P_l: the per-pixel factor 1 / (|f| + eps) is positive, so it cannot move
// a maximum, and rounding it in could only merge two distinct products into a
// tie; labels with and without scores are therefore the same bits, and the
// norm factor is neither loaded nor multiplied when no score is asked for.
// Per pixel and level: one K x 16 NCB product on the decode's A fragments
// (quick_common.h), 768 B read, 4 B (label) + 4 B (score) written.
#include "quick_common.h"

namespace lsr {

#define LSR_SEM_MAX_COLS 256   // 16 projection blocks (64 KB) + the norm factor (16 KB) of the 160 KiB LDS
#define LSR_SEM_NOCOL 0x7fffffff

// 16-lane arg-max of (value, column): the largest value, the lowest column among
// equal values; every lane of each 16-lane row gets its row's pair (the order
// is total, so both lanes of an exchange pick the same pair)
template <int CTRL>
__device__ __forceinline__ void argmax_step(float& v, int& c)
{
    const float pv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
    const int pc = __builtin_amdgcn_update_dpp(0, c, CTRL, 0xF, 0xF, false);
    const bool take = pv > v || (pv == v && pc < c);
    v = take ? pv : v;
    c = take ? pc : c;
}
__device__ __forceinline__ void row16_argmax(float& v, int& c)
{
    argmax_step<0xB1>(v, c);    // quad [1,0,3,2]
    argmax_step<0x4E>(v, c);    // quad [2,3,0,1]
    argmax_step<0x141>(v, c);   // row_half_mirror
    argmax_step<0x140>(v, c);   // row_mirror
}

// Level-resident like k_quick_query: the level's NCB projection blocks (and,
// with SCORE, the 4 norm-factor blocks) stay in LDS, a wave takes 64-pixel
// tiles with the next tile's weights in flight.  A product block leaves its 16
// columns across a row's 16 lanes (lane li = column 16 cb + li, registers =
// pixels 4 lg + r): every lane carries the running best (raw product, column)
// of its own columns through the blocks in ascending order (a later column
// replaces the best only when strictly larger), and one 16-lane arg-max with
// the column as tie-break ends the tile.  SCORE: the lane also carries
// sum_j exp(scale (s_j - m)) against its own running maximum m (rescaled when
// m moves); the lanes' sums are brought to the row's maximum and added.
template <bool SCORE, bool VEC, bool HWC>
__global__ void __launch_bounds__(64 * LSR_DEC2_WAVES, 1)
    k_quick_semantic(const float* __restrict__ wmap, int W, int H, const uint4* __restrict__ pfrag,
                     const float* __restrict__ pscales, const uint4* __restrict__ nfrag,
                     const float* __restrict__ nscales, int* __restrict__ labels, float* __restrict__ scores,
                     float eps, float scale, int nwg, int lk, int n_lab, int n_col, int NCB)
{
    extern __shared__ uint4 sfr[];   // [cb][s][lane][hi, lo] projection, then 4 blocks of the norm factor
    const int l = (int)blockIdx.x / nwg, wi = (int)blockIdx.x % nwg;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
    {
        const uint4* src = pfrag + (size_t)l * NCB * 256;
        for (int i = threadIdx.x; i < NCB * 256; i += 64 * LSR_DEC2_WAVES) sfr[i] = src[i];
        if constexpr (SCORE) {
            const uint4* ns = nfrag + (size_t)l * 4 * 256;
            for (int i = threadIdx.x; i < 4 * 256; i += 64 * LSR_DEC2_WAVES) sfr[NCB * 256 + i] = ns[i];
        }
    }
    __syncthreads();
    const float sc = pscales[l];
    const float ns2 = SCORE ? nscales[l] * nscales[l] : 0.f;
    const size_t HW = (size_t)W * H;
    const int nbx = (W + 63) / 64;
    const int ntile = nbx * H;
    const int stride = nwg * LSR_DEC2_WAVES;
    float raw[4][2][8];
    int t = wi * LSR_DEC2_WAVES + w;
    dec_load_tile<HWC>(raw, wmap, t, ntile, nbx, W, HW, l, lk, li, lg);
    for (; t < ntile; t += stride) {
        const int bx = (t % nbx) * 64, y = t / nbx;
        float psc[4];
        h8 Wh[4][2], Wl[4][2];
        dec_scale_split(raw, psc, Wh, Wl);
        dec_load_tile<HWC>(raw, wmap, t + stride, ntile, nbx, W, HW, l, lk, li, lg);
        // s_j = (w . P_j) mul, both products on the scaled weights w / osc (quick_query.hip)
        float mul[4][4];
        if constexpr (SCORE) {
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
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                const float ipsc = 1.f / psc[pb];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float iosc = __shfl(ipsc, 4 * lg + r, 64);
                    mul[pb][r] = sc / (sqrtf(fmaxf(row16_sum(sq[pb][r]) * ns2, 0.f)) + eps * iosc);
                }
            }
        }
        f32x4q v[4];
        auto products = [&](int cb) {
            const uint4* f = sfr + (size_t)cb * 256 + lane * 2;
            const h8 c0h = __builtin_bit_cast(h8, f[0]), c0l = __builtin_bit_cast(h8, f[1]);
            const h8 c1h = __builtin_bit_cast(h8, f[128]), c1l = __builtin_bit_cast(h8, f[129]);
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                f32x4q acc = {0.f, 0.f, 0.f, 0.f};
                LSR_DEC_MFMA6(acc, pb);
                v[pb] = acc;
            }
        };
        // block 0: every lane with a column (li < n_col) starts from it
        // (its column is 16 * block + li: the block, 4 bits per pixel, is all a lane keeps)
        float best[4][4], sum[4][4];
        unsigned bblk[2] = {0u, 0u};
        const bool has = li < n_col;
        products(0);
#pragma unroll
        for (int pb = 0; pb < 4; pb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                best[pb][r] = has ? v[pb][r] : -INFINITY;
                if constexpr (SCORE) sum[pb][r] = has ? 1.f : 0.f;
            }
#pragma unroll 1
        for (int cb = 1; cb < NCB; cb++) {
            products(cb);
            const int col = 16 * cb + li;
            if (col < n_col) {   // (a lane with a column here had one in block 0: best is finite)
#pragma unroll
                for (int pb = 0; pb < 4; pb++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float p = v[pb][r];
                        const bool up = p > best[pb][r];
                        if constexpr (SCORE) {
                            // d >= 0 when up (a positive factor keeps the order), e = exp(-scale |s_j - m|)
                            const float d = (p - best[pb][r]) * mul[pb][r];
                            const float e = expf(-scale * fabsf(d));
                            sum[pb][r] = up ? fmaf(sum[pb][r], e, 1.f) : sum[pb][r] + e;
                        }
                        best[pb][r] = up ? p : best[pb][r];
                        const int sh = 4 * (4 * (pb & 1) + r);
                        bblk[pb >> 1] = up ? (bblk[pb >> 1] & ~(0xFu << sh)) | ((unsigned)cb << sh) : bblk[pb >> 1];
                    }
            }
        }
        int lab4[4][4];
        float sc4[4][4];
#pragma unroll
        for (int pb = 0; pb < 4; pb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float own = best[pb][r];
                float bv = own;
                int bc = has ? 16 * (int)((bblk[pb >> 1] >> (4 * (4 * (pb & 1) + r))) & 0xFu) + li : LSR_SEM_NOCOL;
                row16_argmax(bv, bc);
                lab4[pb][r] = bc < n_lab ? bc : -1;
                if constexpr (SCORE) {
                    // the lane's sum is against its own maximum own * mul; the row's is bv * mul
                    const float m = mul[pb][r];
                    const float part = has ? sum[pb][r] * expf(-scale * fabsf((bv - own) * m)) : 0.f;
                    sc4[pb][r] = 1.f / row16_sum(part);   // (a division: 1 / (C + N) exactly for the all-zero pixel)
                }
            }
        // lane li = 0 of each row writes the labels of its 4 x 4 pixels, lane li = 1 the scores
        const size_t rowo = (size_t)l * HW + (size_t)y * W;
        if (li == 0) {
#pragma unroll
            for (int pb = 0; pb < 4; pb++) {
                const int xo = bx + 16 * pb + 4 * lg;
                int* o = labels + rowo + xo;
                if (VEC && xo + 3 < W) {
                    *reinterpret_cast<int4*>(o) = make_int4(lab4[pb][0], lab4[pb][1], lab4[pb][2], lab4[pb][3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (xo + r < W) o[r] = lab4[pb][r];
                }
            }
        }
        if constexpr (SCORE) {
            if (li == 1) {
#pragma unroll
                for (int pb = 0; pb < 4; pb++) {
                    const int xo = bx + 16 * pb + 4 * lg;
                    float* o = scores + rowo + xo;
                    if (VEC && xo + 3 < W) {
                        *reinterpret_cast<float4*>(o) = make_float4(sc4[pb][0], sc4[pb][1], sc4[pb][2], sc4[pb][3]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (xo + r < W) o[r] = sc4[pb][r];
                    }
                }
            }
        }
    }
}

// The semantic plan: the query plan's pieces (quick_query.hip) with the label
// columns first: projection fragments (L x NCB x 4 KB) + scales, the norm
// factor chain, and the f32 projection the fragments are packed from.
struct SemPlan {
    uint4* pfrag;
    float* pscales;
    float* G;
    float* Lf;
    uint4* nfrag;
    float* nscales;
    float* P;
    size_t bytes;
};

static SemPlan sem_plan_layout(void* ws, int L, int K, int ncp)
{
    auto up = [](size_t n) { return (n + 255) / 256 * 256; };
    const uintptr_t p = (uintptr_t)ws;   // (nullptr: only .bytes is used)
    SemPlan q;
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

static int sem_ncp(int n_lab, int n_neg) { return (n_lab + n_neg + 15) / 16 * 16; }

size_t quick_semantic_plan_bytes(int L, int K, int n_lab, int n_neg)
{
    return sem_plan_layout(nullptr, L, K, sem_ncp(n_lab, n_neg)).bytes;
}

hipError_t launch_quick_semantic_prepare(const float* cb, const float* lab, const float* neg, int L, int K, int Df,
                                         int n_lab, int n_neg, void* ws, hipStream_t st)
{
    if (L == 0) return hipSuccess;
    const int ncp = sem_ncp(n_lab, n_neg);
    const SemPlan q = sem_plan_layout(ws, L, K, ncp);
    // launch_query_project's columns are its `neg` rows, then its `pos` rows: the labels go first
    launch_query_project(cb, neg, lab, L, K, Df, n_neg, n_lab, ncp, q.P, st);
    launch_codebook_frag(q.P, L, K, ncp, q.pfrag, q.pscales, st);
    norm_factor_prepare(cb, L, K, Df, q.G, q.Lf, q.nfrag, q.nscales, true, st);
    return hipGetLastError();
}

hipError_t launch_quick_semantic_run(const float* wmap, bool hwc, const void* ws, int L, int K, int n_lab, int n_neg,
                                     int H, int W, float scale, float eps, int32_t* labels, float* scores,
                                     hipStream_t st)
{
    if (L == 0 || H == 0 || W == 0) return hipSuccess;
    const int ncp = sem_ncp(n_lab, n_neg);
    const SemPlan q = sem_plan_layout(const_cast<void*>(ws), L, K, ncp);
    const bool score = scores != nullptr;
    const bool vec = (W % 4) == 0 && ((uintptr_t)labels % 16) == 0 && ((uintptr_t)scores % 16) == 0;
    const int ncu = cu_count();
    const int nwg = ncu / L > 0 ? ncu / L : 1;
    const int NCB = ncp / 16;
    const size_t lds = (size_t)(NCB + (score ? 4 : 0)) * 256 * sizeof(uint4);
    with_bools([&](auto scc, auto vecc, auto hwcc) {
        auto kern = k_quick_semantic<scc.value, vecc.value, hwcc.value>;
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        kern<<<(unsigned)(nwg * L), 64 * LSR_DEC2_WAVES, lds, st>>>(wmap, W, H, q.pfrag, q.pscales, q.nfrag, q.nscales,
                                                                   labels, scores, eps, scale, nwg, L * K, n_lab,
                                                                   n_lab + n_neg, NCB);
    }, score, vec, hwc);
    return hipGetLastError();
}

// ---------------------------------------------------------------- level merge

// Per pixel the level with the largest score, the lowest level on ties (a NaN
// score never wins); out = that level's label.  This rule is this project's
// own: the reference returns the per-level maps only.
__global__ void __launch_bounds__(256) k_semantic_merge(const int* __restrict__ labels, const float* __restrict__ scores,
                                                        int L, size_t HW, int* __restrict__ out,
                                                        uint8_t* __restrict__ level)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    float bs = scores[i];
    int bl = 0;
    for (int l = 1; l < L; l++) {
        const float s = scores[(size_t)l * HW + i];
        if (s > bs) {
            bs = s;
            bl = l;
        }
    }
    out[i] = labels[(size_t)bl * HW + i];
    if (level) level[i] = (uint8_t)bl;
}

hipError_t launch_semantic_merge(const int32_t* labels, const float* scores, int L, int H, int W, int32_t* out,
                                 uint8_t* level, hipStream_t st)
{
    const size_t HW = (size_t)H * W;
    if (L == 0 || HW == 0) return hipSuccess;
    k_semantic_merge<<<(unsigned)((HW + 255) / 256), 256, 0, st>>>(labels, scores, L, HW, out, level);
    return hipGetLastError();
}

// ---------------------------------------------------------------- confusion counts

#define LSR_CONF_LDS_COUNTERS 8192   // 32 KB of u32 counters: the table is block-private up to C = 90
#define LSR_CONF_PIX_PER_BLOCK 16384

// counts[p][g][c] += 1 per pixel with gt = g in [0, C) and pred = c in [-1, C)
// (column C collects -1).  LDS: the block counts its pixels (< 2^32) in a
// private u32 table and adds the non-zero entries to the int64 table; else
// every pixel is one 64-bit atomic on the table.  Integer sums: exact and
// the same bits in any order.
template <bool LDS>
__global__ void __launch_bounds__(256) k_semantic_confusion(const int* __restrict__ pred, const int* __restrict__ gt,
                                                            size_t HW, int C, unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned int tab[];
    const int p = blockIdx.y;
    const int n = C * (C + 1);
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < n; i += 256) tab[i] = 0u;
        __syncthreads();
    }
    const int* pr = pred + (size_t)p * HW;
    unsigned long long* ct = counts + (size_t)p * n;
    const size_t i0 = (size_t)blockIdx.x * LSR_CONF_PIX_PER_BLOCK;
    const size_t i1 = i0 + LSR_CONF_PIX_PER_BLOCK < HW ? i0 + LSR_CONF_PIX_PER_BLOCK : HW;
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const int g = gt[i], c = pr[i];
        if (g < 0 || g >= C || c < -1 || c >= C) continue;
        const int e = g * (C + 1) + (c < 0 ? C : c);
        if constexpr (LDS) atomicAdd(&tab[e], 1u);
        else atomicAdd(&ct[e], 1ull);
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) {
            const unsigned int k = tab[i];
            if (k) atomicAdd(&ct[i], (unsigned long long)k);
        }
    }
}

hipError_t launch_semantic_confusion(const int32_t* pred, const int32_t* gt, int P, int H, int W, int C,
                                     int64_t* counts, hipStream_t st)
{
    const size_t HW = (size_t)H * W;
    if (P == 0 || HW == 0) return hipSuccess;
    const size_t n = (size_t)C * (C + 1);
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)P * n * sizeof(int64_t), st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((HW + LSR_CONF_PIX_PER_BLOCK - 1) / LSR_CONF_PIX_PER_BLOCK), (unsigned)P);
    if (n <= LSR_CONF_LDS_COUNTERS)
        k_semantic_confusion<true><<<grid, 256, n * sizeof(unsigned int), st>>>(pred, gt, HW, C,
                                                                                (unsigned long long*)counts);
    else
        k_semantic_confusion<false><<<grid, 256, 0, st>>>(pred, gt, HW, C, (unsigned long long*)counts);
    return hipGetLastError();
}

}  // namespace lsr
