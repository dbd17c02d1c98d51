// kmeans.hip — k-means codebook initialisation of the feature phase: the
// nearest-centre search and the per-cluster means of Lloyd's iteration over the
// (M, D) table of 2-D language features.  Replaces, per level of
// ResidualVectorQuantizationWithClustering.fit_quantizers (utils/vq_utils.py:53-81,
// called from train.py:78-85), the host round trip through
// sklearn.cluster.MiniBatchKMeans and the M x K matrix of
//   torch.cdist(data, centers).argmin(dim=1);  residuals = data - centers[indices]
//
// Assign: score_k = |c_k|^2 - 2 x.c_k on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32, bitwise a sequential fmaf chain): the centres are the
// A operand (16 centres per tile), 16 rows of x the B operand, the accumulator
// starts at |c_k|^2 (formed in f64, rounded once) and A holds -2 c (exact), so a
// score carries D + 1 roundings.  A lane's result registers are 4 centres of one
// row: the argmin runs in the lane over its centres in ascending index order,
// then across the four lanes of the row, ties to the lowest index.  |x|^2 is
// summed in f64 beside the products, dist = max(score + |x|^2, 0) rounded once.
//
// The k order of the MFMA is permuted so that both operands load 16 B per lane:
// k-step j of the 16-dim chunk q takes, in lane group lg, dim 16 q + 4 lg + j.
// Both operands use the same permutation, so the sum is the same set of products
// in a fixed order.
//
// Update: no float atomics.  A workgroup owns a column slice and a row range; a
// thread owns one column of a K x columns LDS tile and walks its rows in order.
// The row ranges depend on (M, K, D) only, the partials are added in index
// order: the means are bit-identical from run to run.
#include <math.h>
#include "lsr_internal.h"

namespace lsr {

namespace {

typedef float f32x4k __attribute__((ext_vector_type(4)));

int km_cu_count()
{
    static int ncu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess)
            (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    return ncu;
}

// centre tiles of 16, padded to a power of two (the compiled accumulator shapes)
int km_tiles(int K)
{
    const int kt = (K + 15) / 16;
    int p = 1;
    while (p < kt) p *= 2;
    return p;
}

// columns (= threads) of an update workgroup: K x columns floats of LDS, at most 64 KB
int km_update_cols(int K) { return K <= 64 ? 256 : K <= 128 ? 128 : 64; }

// The workspace: what depends on the centres first (lsr_kmeans_prepare does not
// know M), then the update's partials.
struct KmWs {
    f32x4k* frag;   // [D/16 chunks][KT tiles][64 lanes]: -2 c[16 t + li][16 q + 4 lg + j], j = 0..3
    float* cn;      // 16 KT: |c_k|^2, +inf for the padding
    float* craw;    // (K, D) copy of the centres (the residual's and an empty cluster's source)
    int* cnt;       // (nparts, K)
    float* part;    // (nparts, K, D)
    int nparts, rpp;
    size_t bytes;
};

KmWs km_layout(const void* ws, int64_t M, int K, int D)
{
    const uintptr_t p = (uintptr_t)ws;   // (nullptr: only .bytes is used)
    const int KT = km_tiles(K), DQ = (D + 15) / 16;
    KmWs w = {};
    size_t o = 0;
    w.frag = (f32x4k*)(p + o); o += align256((size_t)DQ * KT * 64 * 16);
    w.cn = (float*)(p + o);    o += align256((size_t)KT * 16 * 4);
    w.craw = (float*)(p + o);  o += align256((size_t)K * D * 4);
    // row ranges of 1,024 rows, fewer and longer once the partials would pass 64 MB (64 .. 1,024 ranges)
    int64_t maxparts = ((int64_t)64 << 20) / ((int64_t)K * D * 4);
    maxparts = maxparts < 64 ? 64 : maxparts > 1024 ? 1024 : maxparts;
    int64_t rpp = 1024, nparts = (M + rpp - 1) / rpp;
    if (nparts > maxparts) {
        rpp = ((M + maxparts - 1) / maxparts + 7) & ~(int64_t)7;
        nparts = (M + rpp - 1) / rpp;
    }
    w.nparts = (int)nparts;
    w.rpp = (int)rpp;
    w.cnt = (int*)(p + o);    o += align256((size_t)nparts * K * 4);
    w.part = (float*)(p + o); o += align256((size_t)nparts * K * D * 4);
    w.bytes = o;
    return w;
}

}  // namespace

// ---------------------------------------------------------------------------
// Once per centre set: the A-operand fragments, the norms and the raw copy.
__global__ void __launch_bounds__(256) k_km_prepare(const float* __restrict__ c, int K, int D, int KT,
                                                    f32x4k* __restrict__ frag, float* __restrict__ cn,
                                                    float* __restrict__ craw)
{
    const int DQ = (D + 15) / 16;
    const int nth = (int)gridDim.x * 256, g = (int)blockIdx.x * 256 + (int)threadIdx.x;
    for (int e = g; e < DQ * KT * 64; e += nth) {
        const int lane = e & 63, t = (e >> 6) % KT, q = (e >> 6) / KT;
        const int k = 16 * t + (lane & 15), d = 16 * q + 4 * (lane >> 4);
        f32x4k v = {0.f, 0.f, 0.f, 0.f};
        if (k < K && d < D) v = -2.f * *reinterpret_cast<const f32x4k*>(c + (size_t)k * D + d);
        frag[e] = v;
    }
    // |c_k|^2: one wave per centre, f64 (the squares are exact), one rounding to f32
    const int lane = threadIdx.x & 63;
    for (int k = g >> 6; k < 16 * KT; k += nth >> 6) {
        double s = 0.0;
        if (k < K)
            for (int d = lane; d < D; d += 64) {
                const double v = (double)c[(size_t)k * D + d];
                s = fma(v, v, s);
            }
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
        if (lane == 0) cn[k] = k < K ? (float)s : INFINITY;
    }
    for (int e = g; e < K * D / 4; e += nth)
        reinterpret_cast<f32x4k*>(craw)[e] = reinterpret_cast<const f32x4k*>(c)[e];
}

// ---------------------------------------------------------------------------
// One wave = 16 RB rows against all 16 KT centres; persistent waves stride over
// the row tiles.  acc[t][rb][r] = score of centre 16 t + 4 lg + r, row 16 rb + li.
template <int KT, int RB, bool RES>
__global__ void __launch_bounds__(256) k_km_assign(const float* __restrict__ x, int M, int D, int K,
                                                   const f32x4k* __restrict__ frag, const float* __restrict__ cn,
                                                   const float* __restrict__ craw, int* __restrict__ assign,
                                                   float* __restrict__ dist, float* __restrict__ res)
{
    const int lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const int DQ = (D + 15) >> 4;
    constexpr int TR = 16 * RB;
    const int ntile = (int)(((int64_t)M + TR - 1) / TR);
    const int stride = (int)gridDim.x * 4;
    const f32x4k zero = {0.f, 0.f, 0.f, 0.f};
    for (int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); tile < ntile; tile += stride) {
        const int64_t row0 = (int64_t)tile * TR;
        const float* xr[RB];   // a row past the end reads the last row (its results are not stored)
#pragma unroll
        for (int rb = 0; rb < RB; rb++) {
            const int64_t row = row0 + 16 * rb + li;
            xr[rb] = x + (size_t)(row < M ? row : (int64_t)M - 1) * D + 4 * lg;
        }
        f32x4k acc[KT][RB];
#pragma unroll
        for (int t = 0; t < KT; t++) {
            const f32x4k n = *reinterpret_cast<const f32x4k*>(cn + 16 * t + 4 * lg);
#pragma unroll
            for (int rb = 0; rb < RB; rb++) acc[t][rb] = n;
        }
        double xn[RB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++) xn[rb] = 0.0;
        f32x4k xv[RB], av[KT];
        auto load = [&](int q) {
            const bool in = 16 * q + 4 * lg < D;   // D % 4 == 0: a lane's 4 dims are all in or all out
#pragma unroll
            for (int rb = 0; rb < RB; rb++) xv[rb] = in ? *reinterpret_cast<const f32x4k*>(xr[rb] + 16 * q) : zero;
#pragma unroll
            for (int t = 0; t < KT; t++) av[t] = frag[((size_t)q * KT + t) * 64 + lane];
        };
        load(0);
        for (int q = 0; q < DQ; q++) {
            f32x4k xc[RB], ac[KT];
#pragma unroll
            for (int rb = 0; rb < RB; rb++) xc[rb] = xv[rb];
#pragma unroll
            for (int t = 0; t < KT; t++) ac[t] = av[t];
            if (q + 1 < DQ) load(q + 1);   // the next chunk in flight during this one's products
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
#pragma unroll
                for (int j = 0; j < 4; j++) xn[rb] = fma((double)xc[rb][j], (double)xc[rb][j], xn[rb]);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int t = 0; t < KT; t++)
#pragma unroll
                    for (int rb = 0; rb < RB; rb++)
                        acc[t][rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t][j], xc[rb][j], acc[t][rb], 0, 0, 0);
        }
        int best[RB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++) {
            // in the lane: centres in ascending index order, strict <, so the first minimum stays
            float bs = acc[0][rb][0];
            int bi = 4 * lg;
#pragma unroll
            for (int t = 0; t < KT; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float s = acc[t][rb][r];
                    if (s < bs) {
                        bs = s;
                        bi = 16 * t + 4 * lg + r;
                    }
                }
            // across the row's four lanes: the lower score, on a tie the lower index
#pragma unroll
            for (int m = 16; m <= 32; m *= 2) {
                const float s2 = __shfl_xor(bs, m, 64);
                const int i2 = __shfl_xor(bi, m, 64);
                if (s2 < bs || (s2 == bs && i2 < bi)) {
                    bs = s2;
                    bi = i2;
                }
            }
            double n = xn[rb];
            n += __shfl_xor(n, 16, 64);
            n += __shfl_xor(n, 32, 64);
            bi = min(bi, K - 1);   // (all-NaN scores: still a valid centre)
            best[rb] = bi;
            const int64_t row = row0 + 16 * rb + li;
            if (lg == 0 && row < M) {
                assign[row] = bi;
                dist[row] = fmaxf((float)((double)bs + n), 0.f);
            }
        }
        if constexpr (RES) {
            const int D4 = D >> 2;
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
                for (int rr = 0; rr < 16; rr++) {
                    const int64_t row = row0 + 16 * rb + rr;
                    if (row >= M) break;
                    const int idx = __shfl(best[rb], rr, 64);
                    const f32x4k* xs = reinterpret_cast<const f32x4k*>(x + (size_t)row * D);
                    const f32x4k* cs = reinterpret_cast<const f32x4k*>(craw + (size_t)idx * D);
                    f32x4k* o = reinterpret_cast<f32x4k*>(res + (size_t)row * D);
                    for (int d4 = lane; d4 < D4; d4 += 64) o[d4] = xs[d4] - cs[d4];
                }
        }
    }
}

// ---------------------------------------------------------------------------
// Per-cluster sums of one (column slice, row range): thread tid owns column tid
// of the LDS tile, so no two threads touch the same word and the rows are added
// in index order.  The slice-0 workgroup also counts the range's rows per cluster.
__global__ void __launch_bounds__(256) k_km_update(const float* __restrict__ x, const int* __restrict__ assign, int M,
                                                   int D, int K, int rpp, int* __restrict__ cntpart,
                                                   float* __restrict__ part)
{
    extern __shared__ float km_tile[];   // K x CW sums, then K counts
    const int CW = (int)blockDim.x, tid = (int)threadIdx.x;
    const int col = (int)blockIdx.x * CW + tid, p = (int)blockIdx.y;
    const bool act = col < D, counting = blockIdx.x == 0;
    int* lcnt = reinterpret_cast<int*>(km_tile + (size_t)K * CW);
    for (int k = 0; k < K; k++) km_tile[k * CW + tid] = 0.f;
    if (counting)
        for (int k = tid; k < K; k += CW) lcnt[k] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)p * rpp;
    const int64_t r1 = r0 + rpp < (int64_t)M ? r0 + rpp : (int64_t)M;
    const float* xp = x + (act ? col : 0);
    for (int64_t r = r0; r < r1; r += 8) {
        int a[8];
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const bool ok = r + u < r1;
            a[u] = ok ? assign[r + u] : -1;
            v[u] = ok && act ? xp[(size_t)(r + u) * D] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if ((unsigned)a[u] < (unsigned)K) {   // (an index outside [0, K) is skipped, not trusted)
                km_tile[a[u] * CW + tid] += v[u];
                if (counting && tid == 0) lcnt[a[u]]++;
            }
    }
    if (act)
        for (int k = 0; k < K; k++) part[((size_t)p * K + k) * D + col] = km_tile[k * CW + tid];
    __syncthreads();
    if (counting)
        for (int k = tid; k < K; k += CW) cntpart[(size_t)p * K + k] = lcnt[k];
}

// The partials in index order, the division, and an empty cluster's old centre.
__global__ void __launch_bounds__(256) k_km_finish(const float* __restrict__ part, const int* __restrict__ cntpart,
                                                   int nparts, int K, int D, const float* __restrict__ craw,
                                                   float* __restrict__ centers_out, int* __restrict__ counts_out)
{
    __shared__ int scnt;
    const int k = blockIdx.y, d = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (threadIdx.x == 0) scnt = 0;
    __syncthreads();
    int c = 0;
    for (int p = threadIdx.x; p < nparts; p += 256) c += cntpart[(size_t)p * K + k];
    if (c) atomicAdd(&scnt, c);   // (integers: any order gives the same sum)
    __syncthreads();
    const int n = scnt;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts_out[k] = n;
    if (d >= D) return;
    float s = 0.f;
    for (int p = 0; p < nparts; p++) s += part[((size_t)p * K + k) * D + d];
    float o = craw[(size_t)k * D + d];
    if (n > 0) o = n <= (1 << 24) ? s / (float)n : (float)((double)s / (double)n);
    centers_out[(size_t)k * D + d] = o;
}

// ---------------------------------------------------------------------------
size_t kmeans_workspace_bytes(int64_t M, int K, int D) { return km_layout(nullptr, M, K, D).bytes; }

hipError_t launch_kmeans_prepare(const float* centers, int K, int D, void* ws, hipStream_t st)
{
    const KmWs w = km_layout(ws, 0, K, D);
    const int KT = km_tiles(K), DQ = (D + 15) / 16;
    const int work = DQ * KT * 64 > K * D / 4 ? DQ * KT * 64 : K * D / 4;
    int blocks = (work + 255) / 256;
    blocks = blocks < KT * 4 ? KT * 4 : blocks > 256 ? 256 : blocks;   // at least a wave per centre
    k_km_prepare<<<blocks, 256, 0, st>>>(centers, K, D, KT, w.frag, w.cn, w.craw);
    return hipGetLastError();
}

template <int KT, int RB>
static void km_assign_launch(const float* x, int M, int D, int K, const KmWs& w, int* assign, float* dist, float* res,
                             hipStream_t st)
{
    const int64_t ntile = ((int64_t)M + 16 * RB - 1) / (16 * RB);
    // persistent: two workgroups of four waves per CU; a small table gets half as many
    // waves as it has tiles, so every wave still strides
    int64_t blocks = (ntile + 7) / 8;
    blocks = blocks < 1 ? 1 : blocks > 2 * km_cu_count() ? 2 * km_cu_count() : blocks;
    with_bools([&](auto resc) {
        k_km_assign<KT, RB, resc.value><<<(unsigned)blocks, 256, 0, st>>>(x, M, D, K, w.frag, w.cn, w.craw, assign,
                                                                         dist, res);
    }, res != nullptr);
}

hipError_t launch_kmeans_assign(const float* x, int M, int D, int K, const void* ws, int* assign, float* dist,
                                float* residual, hipStream_t st)
{
    if (M == 0) return hipSuccess;
    const KmWs w = km_layout(ws, M, K, D);
    switch (km_tiles(K)) {
    case 1: km_assign_launch<1, 4>(x, M, D, K, w, assign, dist, residual, st); break;
    case 2: km_assign_launch<2, 4>(x, M, D, K, w, assign, dist, residual, st); break;
    case 4: km_assign_launch<4, 4>(x, M, D, K, w, assign, dist, residual, st); break;
    case 8: km_assign_launch<8, 2>(x, M, D, K, w, assign, dist, residual, st); break;
    case 16: km_assign_launch<16, 1>(x, M, D, K, w, assign, dist, residual, st); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kmeans_update(const float* x, const int* assign, int M, int D, int K, void* ws, float* centers_out,
                                int* counts_out, hipStream_t st)
{
    const KmWs w = km_layout(ws, M, K, D);
    const int CW = km_update_cols(K);
    if (w.nparts > 0) {
        const size_t lds = (size_t)K * CW * 4 + (size_t)K * 4;
        (void)hipFuncSetAttribute((const void*)k_km_update, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        k_km_update<<<dim3((unsigned)((D + CW - 1) / CW), (unsigned)w.nparts), CW, lds, st>>>(x, assign, M, D, K, w.rpp,
                                                                                              w.cnt, w.part);
    }
    k_km_finish<<<dim3((unsigned)((D + 255) / 256), (unsigned)K), 256, 0, st>>>(w.part, w.cnt, w.nparts, K, D, w.craw,
                                                                                centers_out, counts_out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the next iteration's fragments and norms
    return launch_kmeans_prepare(centers_out, K, D, ws, st);
}

}  // namespace lsr
