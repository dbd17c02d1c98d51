// clip_tiles.hip — the CLIP input tiles of the preprocess step's kept SAM masks:
// mask2segmap's loop over get_seg_img, pad_img and cv2.resize (preprocess.py:304-317,
// :191-206), then the / 255 of :315 and encode_image's normalisation and cast
// (:105-107, :42-43), read straight from the bit-packed masks of mask_nms.hip.
//
// Boxes: one workgroup per mask strides over its words.  A word may straddle
// image rows (W % 64 != 0), so it is cut into its row segments and each segment
// gives a ctz / clz pair; min / max go through the wave and then LDS.
//
// Tiles: a workgroup owns kTileBand output rows of one tile.  Its first threads
// put the tile's S horizontal taps and coefficients and the band's vertical ones
// in LDS (fp64 for the source coordinate, once per workgroup; the two tables
// share floor(f) and differ at the edges, DESIGN "CLIP tiles").  Then a thread
// produces kTilePx adjacent pixels of one output row: the two taps of a source
// row are neighbours in the frame, so one unaligned 8-byte read of the mask and
// one of the frame serve both (4 reads per output pixel, not 16); then the
// integer blend; and the store, through the caller's (3, 256) table for the two
// float forms, so no float arithmetic touches a pixel.  Consecutive threads hold
// consecutive pixel groups of a row: a wave writes contiguous runs per channel
// plane (16 B per thread as fp32, 8 B as fp16) or 12 contiguous bytes as uint8.
// A tile whose crop is empty, or whose keep entry is outside [0, N), is all
// zeros (the table's entry 0).
#include <limits.h>
#include "lsr_internal.h"

namespace lsr {

namespace {

constexpr int kBoxThreads = 1024;
constexpr int kTileBand = 16;             // output rows per workgroup
constexpr int kTilePx = 4;                // adjacent output pixels per thread
constexpr int kTileMaxS = LSR_TILE_MAX_SIDE;

// ------------------------------------------------------------------ boxes ---
__global__ void __launch_bounds__(kBoxThreads) k_mask_boxes(const unsigned long long* __restrict__ words, int W,
                                                             int W64, int* __restrict__ boxes)
{
    __shared__ int s_red[4][kBoxThreads / 64];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long* src = words + (size_t)n * W64;
    int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
    for (int i = threadIdx.x; i < W64; i += kBoxThreads) {
        unsigned long long w = src[i];
        if (!w) continue;
        int y = (i * 64) / W, x = i * 64 - y * W, rem = 64;   // bit 0 of w is pixel (y, x); 64 i < 2^24 + 64
        while (w) {
            const int len = min(W - x, rem);                  // this row's share of the word
            const unsigned long long seg = len >= 64 ? w : (w & ((1ull << len) - 1ull));
            if (seg) {
                xmin = min(xmin, x + (int)__builtin_ctzll(seg));
                xmax = max(xmax, x + 63 - (int)__builtin_clzll(seg));
                ymin = min(ymin, y);
                ymax = max(ymax, y);
            }
            w = len >= 64 ? 0ull : (w >> len);
            rem -= len;
            x = 0;
            ++y;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, d));
        ymin = min(ymin, __shfl_xor(ymin, d));
        xmax = max(xmax, __shfl_xor(xmax, d));
        ymax = max(ymax, __shfl_xor(ymax, d));
    }
    if (lane == 0) {
        s_red[0][wave] = xmin;
        s_red[1][wave] = ymin;
        s_red[2][wave] = xmax;
        s_red[3][wave] = ymax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBoxThreads / 64; ++k) {
            xmin = min(xmin, s_red[0][k]);
            ymin = min(ymin, s_red[1][k]);
            xmax = max(xmax, s_red[2][k]);
            ymax = max(ymax, s_red[3][k]);
        }
        int* b = boxes + 4 * (size_t)n;
        const bool any = xmax >= 0;
        b[0] = any ? xmin : 0;
        b[1] = any ? ymin : 0;
        b[2] = any ? xmax - xmin + 1 : 0;
        b[3] = any ? ymax - ymin + 1 : 0;
    }
}

// ------------------------------------------------------------------ tiles ---
__device__ __forceinline__ int clampi(long long v, int lo, int hi) { return (int)(v < lo ? lo : v > hi ? hi : v); }

// Pixels p and p + 1 of the frame, 0 <= p < HW: their mask bits in bits 0 and 1 (pixel HW reads as garbage,
// the caller ignores it) from one unaligned 8-byte read of the mask's words.  The read starts at byte p / 8
// or, where that would pass the mask's 8 W64 bytes, at its last word; bits p and p + 1 then still lie inside.
__device__ __forceinline__ uint32_t load_bits2(const unsigned long long* __restrict__ mw, int W64, int p)
{
    const int at = min(p >> 3, 8 * W64 - 8);
    unsigned long long v;
    __builtin_memcpy(&v, (const uint8_t*)mw + at, 8);
    return (uint32_t)(v >> (p - 8 * at)) & 3u;
}

// Their bytes, pixel p in bits 0-23 and p + 1 in bits 24-47 (garbage for pixel HW), from one unaligned
// 8-byte read of the frame that starts at byte 3 p - 1, clamped into the frame's n3 = 3 HW bytes; frames
// of one or two pixels are read by bytes.
__device__ __forceinline__ unsigned long long load_rgb2(const uint8_t* __restrict__ image, int n3, int p)
{
    unsigned long long v = 0;
    if (n3 >= 8) {
        const int at = min(max(3 * p - 1, 0), n3 - 8);   // 3 p - at <= 2, or p = HW - 1 and its 3 bytes end the read
        __builtin_memcpy(&v, image + at, 8);
        return v >> (8 * (3 * p - at));
    }
    for (int k = 0; k < 6 && 3 * p + k < n3; ++k) v |= (unsigned long long)image[3 * p + k] << (8 * k);
    return v;
}

template <typename T>
__device__ __forceinline__ T tile_value(const T* s_lut, int c, int v)
{
    if constexpr (std::is_same<T, uint8_t>::value) return (uint8_t)v;
    else return s_lut[256 * c + v];
}

// T: uint8_t ("u8", (n, S, S, 3)), float ("unit") or uint16_t (fp16 bits, "clip"), both (n, 3, S, S)
template <typename T>
__global__ void __launch_bounds__(256) k_clip_tiles(const uint8_t* __restrict__ image, int W,
                                                    const unsigned long long* __restrict__ words, int N, int W64,
                                                    const int* __restrict__ keep, const int* __restrict__ boxes,
                                                    int H, int S, const T* __restrict__ lut, bool wide,
                                                    T* __restrict__ out)
{
    __shared__ int s_c0[kTileMaxS];
    __shared__ short s_a0[kTileMaxS], s_a1[kTileMaxS];
    __shared__ int s_r0[kTileBand], s_r1[kTileBand];
    __shared__ short s_b0[kTileBand], s_b1[kTileBand];
    __shared__ T s_lut[std::is_same<T, uint8_t>::value ? 1 : 768];
    const int tid = threadIdx.x, t = blockIdx.y, row0 = blockIdx.x * kTileBand;
    const int rows = min(kTileBand, S - row0);
    const int m = keep ? keep[t] : t;
    int x0 = 0, y0 = 0, cw = 0, ch = 0;
    if ((unsigned)m < (unsigned)N) {   // the box clipped to the frame, as numpy slicing clips it
        const int* b = boxes + 4 * (size_t)m;
        const long long bx = b[0], by = b[1], bw = b[2], bh = b[3];
        x0 = clampi(bx, 0, W);
        y0 = clampi(by, 0, H);
        cw = max(clampi(bx + bw, 0, W) - x0, 0);
        ch = max(clampi(by + bh, 0, H) - y0, 0);
    }
    const int l = max(cw, ch);
    const int ox_off = ch > cw ? (ch - cw) / 2 : 0, oy_off = ch > cw ? 0 : (cw - ch) / 2;
    if constexpr (!std::is_same<T, uint8_t>::value)
        for (int k = tid; k < 768; k += 256) s_lut[k] = lut[k];
    if (l > 0) {
        const double scale = 1.0 / ((double)S / (double)l);
        for (int d = tid; d < S; d += 256) {
            float f = (float)(((double)d + 0.5) * scale - 0.5);
            int s = (int)floorf(f);
            f = f - (float)s;
            if (s < 0) { f = 0.f; s = 0; }
            if (s >= l - 1) { f = 0.f; s = l - 1; }
            s_c0[d] = s;
            s_a0[d] = (short)(int)rintf((1.f - f) * 2048.f);
            s_a1[d] = (short)(int)rintf(f * 2048.f);
        }
        if (tid < rows) {
            float f = (float)(((double)(row0 + tid) + 0.5) * scale - 0.5);
            const int s = (int)floorf(f);
            f = f - (float)s;
            s_r0[tid] = min(max(s, 0), l - 1);
            s_r1[tid] = min(max(s + 1, 0), l - 1);
            s_b0[tid] = (short)(int)rintf((1.f - f) * 2048.f);
            s_b1[tid] = (short)(int)rintf(f * 2048.f);
        }
    }
    __syncthreads();
    const unsigned long long* mw = words + (size_t)((unsigned)m < (unsigned)N ? m : 0) * W64;
    const int groups = (S + kTilePx - 1) / kTilePx;
    const size_t plane = (size_t)S * S;
    T* dst = out + (size_t)t * 3 * plane;
    for (int g = tid; g < rows * groups; g += 256) {
        const int ry = g / groups, ox = (g - ry * groups) * kTilePx, oy = row0 + ry;
        int v[kTilePx][3] = {};
        if (l > 0) {
            const int b0 = s_b0[ry], b1 = s_b1[ry];
            // per source row: is it inside the crop, and the frame pixel index of square column 0
            const int cy0 = s_r0[ry] - oy_off, cy1 = s_r1[ry] - oy_off;
            const bool in0 = (unsigned)cy0 < (unsigned)ch, in1 = (unsigned)cy1 < (unsigned)ch;
            const int base0 = in0 ? (y0 + cy0) * W + x0 - ox_off : 0, base1 = in1 ? (y0 + cy1) * W + x0 - ox_off : 0;
            // The taps at square columns c and c + 1 of one source row, the first in bits 0-23 and the second in
            // bits 24-47; a tap outside the crop or with its mask bit clear is 0.  (Where the table's second tap is
            // c itself, at the square's last column, its coefficient is 0, so reading it as column c + 1 = outside
            // changes nothing.)  The two taps are neighbours in the frame: one read of the mask and one of the frame
            // serve both, anchored on the first of them that lies inside the crop.
            auto taps = [&](bool row_in, int base, int c) -> unsigned long long {
                const int col = c - ox_off;
                const bool first = row_in && (unsigned)col < (unsigned)cw;
                const bool second = row_in && (unsigned)(col + 1) < (unsigned)cw;
                if (!first && !second) return 0ull;
                const int p = base + c + (first ? 0 : 1);   // inside the crop, so inside the frame
                const uint32_t bits = load_bits2(mw, W64, p);
                const unsigned long long px = load_rgb2(image, 3 * H * W, p);
                if (!first) return (bits & 1u) ? (px & 0xffffffull) << 24 : 0ull;
                return ((bits & 1u) ? (px & 0xffffffull) : 0ull) |
                       ((second && (bits & 2u)) ? (px & 0xffffff000000ull) : 0ull);
            };
#pragma unroll
            for (int j = 0; j < kTilePx; ++j) {
                if (ox + j >= S) break;
                const int c0 = s_c0[ox + j];
                const int a0 = s_a0[ox + j], a1 = s_a1[ox + j];
                const unsigned long long t0 = taps(in0, base0, c0), t1 = taps(in1, base1, c0);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int sh = 8 * c;
                    const int h0 = (int)((t0 >> sh) & 255u) * a0 + (int)((t0 >> (sh + 24)) & 255u) * a1;
                    const int h1 = (int)((t1 >> sh) & 255u) * a0 + (int)((t1 >> (sh + 24)) & 255u) * a1;
                    v[j][c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                }
            }
        }
        const bool full = wide && ox + kTilePx <= S;
        if constexpr (std::is_same<T, uint8_t>::value) {
            uint8_t* q = dst + ((size_t)oy * S + ox) * 3;
            if (full) {   // 12 bytes, 4-B aligned: S % 4 == 0
                uint32_t* q4 = (uint32_t*)q;
                q4[0] = (uint32_t)v[0][0] | ((uint32_t)v[0][1] << 8) | ((uint32_t)v[0][2] << 16) | ((uint32_t)v[1][0] << 24);
                q4[1] = (uint32_t)v[1][1] | ((uint32_t)v[1][2] << 8) | ((uint32_t)v[2][0] << 16) | ((uint32_t)v[2][1] << 24);
                q4[2] = (uint32_t)v[2][2] | ((uint32_t)v[3][0] << 8) | ((uint32_t)v[3][1] << 16) | ((uint32_t)v[3][2] << 24);
            } else {
                for (int j = 0; j < kTilePx && ox + j < S; ++j)
                    for (int c = 0; c < 3; ++c) q[3 * j + c] = (uint8_t)v[j][c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                T* q = dst + c * plane + (size_t)oy * S + ox;
                if (full) {
                    struct alignas(4 * sizeof(T)) Quad { T e[4]; } quad;
#pragma unroll
                    for (int j = 0; j < kTilePx; ++j) quad.e[j] = tile_value<T>(s_lut, c, v[j][c]);
                    *(Quad*)q = quad;
                } else {
                    for (int j = 0; j < kTilePx && ox + j < S; ++j) q[j] = tile_value<T>(s_lut, c, v[j][c]);
                }
            }
        }
    }
}

template <typename T>
hipError_t launch_tiles_as(const uint8_t* image, int H, int W, const unsigned long long* words, int N, const int* keep,
                           const int* boxes, int n, int S, const void* lut, void* out, hipStream_t st)
{
    // the wide stores need S % 4 == 0 (every row of every plane starts on the store's alignment) and an aligned base
    const bool wide = S % kTilePx == 0 && ((uintptr_t)out % 16) == 0;
    dim3 grid((S + kTileBand - 1) / kTileBand, n);
    hipLaunchKernelGGL(k_clip_tiles<T>, grid, dim3(256), 0, st, image, W, words, N, (H * W + 63) / 64, keep, boxes, H,
                       S, (const T*)lut, wide, (T*)out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mask_boxes(const unsigned long long* words, int N, int H, int W, int* boxes, hipStream_t st)
{
    hipLaunchKernelGGL(k_mask_boxes, dim3(N), dim3(kBoxThreads), 0, st, words, W, (H * W + 63) / 64, boxes);
    return hipGetLastError();
}

hipError_t launch_clip_tiles(const uint8_t* image, int H, int W, const unsigned long long* words, int N,
                             const int* keep, const int* boxes, int n, int S, const void* lut, int out_type, void* out,
                             hipStream_t st)
{
    if (out_type == LSR_TILE_U8)
        return launch_tiles_as<uint8_t>(image, H, W, words, N, keep, boxes, n, S, nullptr, out, st);
    if (out_type == LSR_TILE_UNIT)
        return launch_tiles_as<float>(image, H, W, words, N, keep, boxes, n, S, lut, out, st);
    return launch_tiles_as<uint16_t>(image, H, W, words, N, keep, boxes, n, S, lut, out, st);
}

}  // namespace lsr
