// mask_nms.hip — the tensor part of the preprocess step that writes <image>_s.npy:
// mask_nms (preprocess.py:215-279) and mask2segmap with create's level offsets
// (preprocess.py:304-317, :145-157).  The reference walks all N (N + 1) / 2 mask
// pairs in Python with several full-frame reductions per pair; here the masks
// are bit-packed once and every pair quantity is an integer popcount.
//
// Pack: one wave packs 64 pixels with one ballot; bit b of word w is pixel
// 64 w + b in row-major order, bits past H W are zero.  The areas are the
// popcounts of the same ballots, added with integer atomics.  Rows of 16-B
// aligned bytes are loaded 16 pixels per lane and turned through LDS.
//
// Pair counts: inter[i][j] = sum_w popcount(words[i][w] & words[j][w]) for ranks
// i <= j.  A workgroup owns a 64 x 64 tile of pairs (upper-triangle tiles only)
// and a range of 32-word chunks; it stages the 2 x 64 x 32 words of a chunk in
// LDS once and each of its 256 threads holds a 4 x 4 register tile, so a word
// read from LDS serves 4 pairs.  Integer atomics only: the table is exact and
// the same from run to run however the word axis is split.
//
// Decide: column maxima of the three float matrices straight from inter and
// area, the keep rule, the fallbacks and the ordered compaction in one launch;
// the last workgroup to finish (a ticket) does the part that needs every column.
//
// Segment maps: one thread per pixel and level scans the level's kept list from
// the back and stops at the first mask that covers the pixel.
//
// All float work is plain IEEE fp32 (/, *, -; the Makefile sets -ffp-contract=off)
// and the maxima propagate NaN as torch.max does.
#include "lsr_internal.h"

namespace lsr {

namespace {

constexpr int kPairTile = LSR_MASK_PAIR_TILE;     // masks per side of a pair tile
constexpr int kWordChunk = LSR_MASK_WORD_CHUNK;   // 64-bit words of every mask staged per step
constexpr int kRowStride = kWordChunk + 1;        // LDS row stride in words: rows 66 dwords apart, see DESIGN
constexpr int kPackWords = 8;                     // words a wave packs per step (one 64-B store)
constexpr int kPackSteps = 4;
constexpr int kPackBlockWords = 4 * kPackWords * kPackSteps;   // 4 waves: 128 words = 8192 pixels per workgroup
constexpr int kDecideCols = 32;                   // columns per decide workgroup

int mask_cu_count()
{
    static int ncu = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess)
            (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    return ncu;
}

// torch.max: a NaN on either side wins
__device__ __forceinline__ float nan_max(float m, float v) { return (m != m) ? m : ((v != v) || v > m) ? v : m; }

// ------------------------------------------------------------------- pack ---
__global__ void __launch_bounds__(256) k_mask_pack(const uint8_t* __restrict__ masks, int HW, int W64,
                                                   unsigned long long* __restrict__ words, int* __restrict__ area)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const uint8_t* src = masks + (size_t)n * HW;
    unsigned long long* dst = words + (size_t)n * W64;
    int sum = 0;   // wave-uniform
    for (int s = 0; s < kPackSteps; ++s) {
        const int w0 = blockIdx.x * kPackBlockWords + (wave * kPackSteps + s) * kPackWords;
        if (w0 >= W64) break;
        uint8_t v[kPackWords];
#pragma unroll
        for (int k = 0; k < kPackWords; ++k) {
            const int p = (w0 + k) * 64 + lane;   // < 2^24 + 64 * 8 * 16
            v[k] = p < HW ? src[p] : (uint8_t)0;
        }
        unsigned long long mine = 0;
#pragma unroll
        for (int k = 0; k < kPackWords; ++k) {
            const unsigned long long b = __ballot(v[k] != 0);
            sum += __popcll(b);
            if (lane == k) mine = b;
        }
        if (lane < kPackWords && w0 + lane < W64) dst[w0 + lane] = mine;
    }
    __shared__ int s_sum[4];
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (t) atomicAdd(&area[n], t);
    }
}

// The same for rows of 16-B aligned bytes (H W a multiple of 16): a lane loads 16
// pixels at once, the wave turns its 1024 bytes through LDS so that lane l of
// ballot k again holds pixel 64 k + l.  One byte per lane and load, as above,
// is bound by the load rate, not by the bytes.
constexpr int kWideWords = 16;                    // words a wave packs per step: 64 lanes x 16 B
constexpr int kWideSteps = kPackBlockWords / (4 * kWideWords);

__global__ void __launch_bounds__(256) k_mask_pack_wide(const uint8_t* __restrict__ masks, int HW, int W64,
                                                        unsigned long long* __restrict__ words,
                                                        int* __restrict__ area)
{
    __shared__ uint4 s_px[kWideSteps][4][64];
    __shared__ int s_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.y;
    const uint8_t* src = masks + (size_t)n * HW;
    unsigned long long* dst = words + (size_t)n * W64;
    const int wb = blockIdx.x * kPackBlockWords + wave * kWideSteps * kWideWords;
#pragma unroll
    for (int s = 0; s < kWideSteps; ++s) {
        const int p = (wb + s * kWideWords) * 64 + 16 * lane;   // HW % 16 == 0: p < HW covers p + 15
        s_px[s][wave][lane] = p < HW ? *(const uint4*)(src + p) : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    int sum = 0;   // wave-uniform
#pragma unroll
    for (int s = 0; s < kWideSteps; ++s) {
        const int w0 = wb + s * kWideWords;
        const uint8_t* px = (const uint8_t*)s_px[s][wave];
        unsigned long long mine = 0;
#pragma unroll
        for (int k = 0; k < kWideWords; ++k) {
            const unsigned long long b = __ballot(px[64 * k + lane] != 0);
            sum += __popcll(b);
            if (lane == k) mine = b;
        }
        if (lane < kWideWords && w0 + lane < W64) dst[w0 + lane] = mine;
    }
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        if (t) atomicAdd(&area[n], t);
    }
}

// ------------------------------------------------------------ pair counts ---
// grid.x: upper-triangle tile (ti <= tj), grid.y: split of the word axis
__global__ void __launch_bounds__(256) k_mask_pairs(const unsigned long long* __restrict__ words, int N, int W64,
                                                    const int* __restrict__ order, int tiles, int chunks_per_block,
                                                    int* __restrict__ inter)
{
    __shared__ unsigned long long s_w[2 * kPairTile * kRowStride];
    __shared__ int s_row[2 * kPairTile];   // the mask's row in words, -1 past N
    int ti = 0, rest = blockIdx.x;
    while (rest >= tiles - ti) { rest -= tiles - ti; ++ti; }
    const int tj = ti + rest;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < 2 * kPairTile) {
        const int r = (tid < kPairTile ? ti : tj) * kPairTile + (tid & (kPairTile - 1));
        const int o = r < N ? (order ? order[r] : r) : -1;
        s_row[tid] = (unsigned)o < (unsigned)N ? o : -1;   // an index outside [0, N) reads as an empty mask
    }
    __syncthreads();
    // a thread stages 16 words per chunk: word (tid & 31) of masks (tid >> 5) + 8 k
    constexpr int kStage = 2 * kPairTile * kWordChunk / 256;
    const int sw = tid & (kWordChunk - 1), sm = tid >> 5;
    int rows[kStage];
#pragma unroll
    for (int k = 0; k < kStage; ++k) rows[k] = s_row[sm + 8 * k];
    const int c_begin = blockIdx.y * chunks_per_block;
    const int c_total = (W64 + kWordChunk - 1) / kWordChunk;
    const int c_end = min(c_begin + chunks_per_block, c_total);
    unsigned long long nxt[kStage];
    auto fetch = [&](int c) {
        const int w = c * kWordChunk + sw;
#pragma unroll
        for (int k = 0; k < kStage; ++k) nxt[k] = (rows[k] >= 0 && w < W64) ? words[(size_t)rows[k] * W64 + w] : 0ull;
    };
    int acc[4][4] = {};
    if (c_begin < c_end) fetch(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        __syncthreads();   // the previous chunk is consumed
#pragma unroll
        for (int k = 0; k < kStage; ++k) s_w[(sm + 8 * k) * kRowStride + sw] = nxt[k];
        __syncthreads();
        if (c + 1 < c_end) fetch(c + 1);   // in flight during the popcounts
        const unsigned long long* pa = s_w + ty * kRowStride;
        const unsigned long long* pb = s_w + (kPairTile + tx) * kRowStride;
#pragma unroll 4
        for (int w = 0; w < kWordChunk; ++w) {
            unsigned long long a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = pa[16 * q * kRowStride + w];
                b[q] = pb[16 * q * kRowStride + w];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] += __popcll(a[p] & b[q]);
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = ti * kPairTile + ty + 16 * p, j = tj * kPairTile + tx + 16 * q;
            if (i <= j && j < N && acc[p][q] != 0) atomicAdd(&inter[(size_t)i * N + j], acc[p][q]);
        }
}

// ----------------------------------------------------------------- decide ---
enum { kCritIou = 1, kCritConf = 2, kCritInnerU = 4, kCritInnerL = 8 };

__global__ void __launch_bounds__(256) k_mask_decide(const int* __restrict__ inter, const int* __restrict__ area,
                                                     const int* __restrict__ order, const uint8_t* __restrict__ conf,
                                                     int N, float iou_thr, float inner_cut, uint8_t* crit_ws,
                                                     int* ticket, uint8_t* __restrict__ keep,
                                                     uint8_t* __restrict__ criteria, long long* __restrict__ selected,
                                                     int* __restrict__ count)
{
    __shared__ int s_area[LSR_MASK_MAX_N];   // in rank order
    __shared__ float s_iou[8][kDecideCols], s_u[8][kDecideCols], s_ulast[kDecideCols], s_l[kDecideCols];
    __shared__ int s_scan[256];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    for (int r = tid; r < N; r += 256) {
        const int o = order ? order[r] : r;
        s_area[r] = (unsigned)o < (unsigned)N ? area[o] : 0;
    }
    if (tid < kDecideCols) s_ulast[tid] = 0.0f;
    __syncthreads();
    const int c0 = blockIdx.x * kDecideCols;
    {   // columns: iou and the upper inner matrix, rows i < c
        const int tx = tid & (kDecideCols - 1), ty = tid >> 5, c = c0 + tx;
        float iou_m = 0.0f, u_m = 0.0f;
        if (c < N) {
            const int Ac = s_area[c];
            const float fAc = (float)Ac;
            for (int i = ty; i < c; i += 8) {
                const int I = inter[(size_t)i * N + c], Ai = s_area[i];
                const float fI = (float)I;
                const float iou = fI / (float)(Ai + Ac - I);
                const float a = fI / (float)Ai, b = fI / fAc;
                iou_m = nan_max(iou_m, iou);
                if (a < 0.5f && b >= 0.85f) {
                    const float u = 1.0f - b * a;
                    u_m = nan_max(u_m, u);
                    if (i == c - 1) s_ulast[tx] = u;   // the superdiagonal tril(diagonal=1) keeps
                }
            }
        }
        s_iou[ty][tx] = iou_m;
        s_u[ty][tx] = u_m;
    }
    {   // rows: the lower inner matrix, L[j][c] for j > c comes from inter[c][j]
        const int lane = tid & 63, wave = tid >> 6;
        for (int r = wave; r < kDecideCols; r += 4) {
            const int c = c0 + r;
            float l_m = 0.0f;
            if (c < N) {
                const float fAc = (float)s_area[c];
                for (int j = c + 1 + lane; j < N; j += 64) {
                    const float fI = (float)inter[(size_t)c * N + j];
                    const float a = fI / fAc, b = fI / (float)s_area[j];
                    if (a >= 0.85f && b < 0.5f) l_m = nan_max(l_m, 1.0f - b * a);
                }
            }
            for (int d = 32; d > 0; d >>= 1) l_m = nan_max(l_m, __shfl_xor(l_m, d));
            if (lane == 0) s_l[r] = l_m;
        }
    }
    __syncthreads();
    if (tid < kDecideCols && c0 + tid < N) {
        float iou_m = s_iou[0][tid], u_m = s_u[0][tid];
        for (int k = 1; k < 8; ++k) {
            iou_m = nan_max(iou_m, s_iou[k][tid]);
            u_m = nan_max(u_m, s_u[k][tid]);
        }
        const float l_m = nan_max(s_l[tid], s_ulast[tid]);
        crit_ws[c0 + tid] = (uint8_t)((iou_m <= iou_thr ? kCritIou : 0) | (u_m <= inner_cut ? kCritInnerU : 0) |
                                      (l_m <= inner_cut ? kCritInnerL : 0));
    }
    // the last workgroup to arrive sees every column
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (tid == 0) *ticket = 0;   // ready for the next call
    const volatile uint8_t* crit = crit_ws;
    const int per = (N + 255) / 256, r0 = tid * per, r1 = min(r0 + per, N);
    int any = 0;
    for (int r = r0; r < r1; ++r) any |= (crit[r] & (kCritInnerU | kCritInnerL)) | (conf[r] ? kCritConf : 0);
    const bool any_conf = __syncthreads_or(any & kCritConf), any_u = __syncthreads_or(any & kCritInnerU),
               any_l = __syncthreads_or(any & kCritInnerL);
    // a criterion no rank passes falls back to the three best ranks
    auto flags = [&](int r) {
        int f = crit[r] | (conf[r] ? kCritConf : 0);
        if (!any_conf && r < 3) f |= kCritConf;
        if (!any_u && r < 3) f |= kCritInnerU;
        if (!any_l && r < 3) f |= kCritInnerL;
        return f;
    };
    int mine = 0;
    for (int r = r0; r < r1; ++r) mine += flags(r) == 15;
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int pos = s_scan[tid] - mine;
    for (int r = r0; r < r1; ++r) {
        const int f = flags(r);
        keep[r] = f == 15;
        if (criteria) criteria[r] = (uint8_t)f;
        if (f == 15) selected[pos++] = order ? order[r] : r;
    }
    if (tid == 255) *count = s_scan[255];
}

// ----------------------------------------------------------- segment maps ---
struct SegLevels {
    const unsigned long long* words[4];
    const int* kept[4];
    int masks[4], count[4], offset[4];
};

template <typename T>
__global__ void __launch_bounds__(256) k_mask_segmaps(SegLevels lv, int HW, int W64, T* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (p >= HW) return;
    const unsigned long long* wp = lv.words[l] + (p >> 6);   // one word per wave
    const int* kept = lv.kept[l];
    const int bit = p & 63, nm = lv.masks[l];
    int v = -1;
    for (int k = lv.count[l] - 1; k >= 0; --k) {
        const int m = kept[k];
        if ((unsigned)m < (unsigned)nm && ((wp[(size_t)m * W64] >> bit) & 1ull)) {
            v = k + lv.offset[l];
            break;
        }
    }
    out[(size_t)l * HW + p] = (T)v;
}

}  // namespace

size_t mask_nms_inter_bytes(int N) { return ((size_t)N * N * sizeof(int) + 255) & ~(size_t)255; }

size_t mask_nms_workspace_bytes(int N)
{
    // inter (N, N) int32 | per-rank criteria bits | ticket
    return mask_nms_inter_bytes(N) + (((size_t)N + 255) & ~(size_t)255) + 256;
}

hipError_t launch_mask_pack(const uint8_t* masks, int N, int HW, unsigned long long* words, int* area, hipStream_t st)
{
    const int W64 = (HW + 63) / 64;
    hipError_t e = hipMemsetAsync(area, 0, (size_t)N * sizeof(int), st);
    if (e != hipSuccess) return e;
    dim3 grid((W64 + kPackBlockWords - 1) / kPackBlockWords, N);
    if (HW % 16 == 0 && ((uintptr_t)masks & 15) == 0)
        hipLaunchKernelGGL(k_mask_pack_wide, grid, dim3(256), 0, st, masks, HW, W64, words, area);
    else
        hipLaunchKernelGGL(k_mask_pack, grid, dim3(256), 0, st, masks, HW, W64, words, area);
    return hipGetLastError();
}

hipError_t launch_mask_pairs(const unsigned long long* words, int N, int W64, const int* order, int* inter,
                             hipStream_t st)
{
    hipError_t e = hipMemsetAsync(inter, 0, (size_t)N * N * sizeof(int), st);
    if (e != hipSuccess) return e;
    const int tiles = (N + kPairTile - 1) / kPairTile, ntile = tiles * (tiles + 1) / 2;
    const int chunks = (W64 + kWordChunk - 1) / kWordChunk;
    // four workgroups per CU (LDS), at least 8 chunks each so the final atomics stay a small part
    int split = (4 * mask_cu_count() + ntile - 1) / ntile;
    split = max(1, min(split, chunks / 8));
    const int per = (chunks + split - 1) / split;
    split = (chunks + per - 1) / per;
    hipLaunchKernelGGL(k_mask_pairs, dim3(ntile, split), dim3(256), 0, st, words, N, W64, order, tiles, per, inter);
    return hipGetLastError();
}

hipError_t launch_mask_decide(const int* area, int N, const int* order, const uint8_t* conf, float iou_thr,
                              float inner_cut, void* ws, uint8_t* keep, uint8_t* criteria, long long* selected,
                              int* count, hipStream_t st)
{
    uint8_t* crit = (uint8_t*)ws + mask_nms_inter_bytes(N);
    int* ticket = (int*)((uint8_t*)ws + mask_nms_workspace_bytes(N) - 256);
    hipError_t e = hipMemsetAsync(ticket, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mask_decide, dim3((N + kDecideCols - 1) / kDecideCols), dim3(256), 0, st, (const int*)ws, area,
                       order, conf, N, iou_thr, inner_cut, crit, ticket, keep, criteria, selected, count);
    return hipGetLastError();
}

hipError_t launch_mask_segmaps(const unsigned long long* const* words, const int* const* kept, const int* masks,
                               const int* counts, const int* offsets, int HW, bool as_int, void* out, hipStream_t st)
{
    SegLevels lv;
    for (int l = 0; l < 4; ++l) {
        lv.words[l] = words[l];
        lv.kept[l] = kept[l];
        lv.masks[l] = masks[l];
        lv.count[l] = counts[l];
        lv.offset[l] = offsets[l];
    }
    const int W64 = (HW + 63) / 64;
    dim3 grid((HW + 255) / 256, 4);
    if (as_int)
        hipLaunchKernelGGL(k_mask_segmaps<int>, grid, dim3(256), 0, st, lv, HW, W64, (int*)out);
    else
        hipLaunchKernelGGL(k_mask_segmaps<float>, grid, dim3(256), 0, st, lv, HW, W64, (float*)out);
    return hipGetLastError();
}

}  // namespace lsr
