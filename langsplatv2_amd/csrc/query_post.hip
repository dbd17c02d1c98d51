// query_post.hip — the post-process every caller of get_max_across_quick runs
// on the (L, Q, H, W) relevancy maps (eval_lerf.py:111-200, eval_3d_ovs.py:
// 102-107, 215-260), on planes = L * Q independent H x W fp32 planes:
//
//   smooth pass  k x k box mean with the window clipped to the image
//                (AvgPool2d(k, 1, (k - 1) / 2, count_include_pad=False)),
//                blend = 0.5 (avg + v), per-tile {min, max of blend; max of avg,
//                its first row-major pixel, how many pixels attain it}
//   finish       the tile partials of a plane, in a fixed order
//   mask pass    o = clip(2 (blend - min) / (max - min + 1e-9) - 1, 0, 1),
//                raw = o > thresh, mask = majority of raw over the clipped
//                (2 s + 1)^2 window, per-tile {area, intersection and union
//                with an annotation mask, sum of blend over the mask}
//   finish       the same for the mask pass's partials
//
// Separate launches order the passes; there is no float atomic and no atomic
// at all, so every output is bit-identical from run to run.
//
// Box sum: a 32 x 64 tile plus an r halo is staged in LDS with zeros outside
// the image (adding 0.0f is exact), then row sums of 2 r + 1 terms, then column
// sums of 2 r + 1 row sums.  Every window is summed on its own (no running sum
// along a row or column), so the error does not grow with the image: the 29-tap
// kernel adds each window as a fixed tree (window29: a tap passes through at
// most 7 + 7 rounded additions), the others in order (2 r + 2 r additions).
#include "lsr_internal.h"

namespace lsr {
namespace {

constexpr int QP_TH = 32, QP_TW = 64, QP_THREADS = 256, QP_STRIP = 8;
constexpr int QP_WAVES = QP_THREADS / 64;
static_assert(QP_TH == QP_WAVES * QP_STRIP, "one 8-row strip of the tile per wave");

struct SmoothPartial {
    float bmin, bmax, amax;
    uint32_t idx, cnt;
};
struct MaskPartial {
    double msum;
    uint32_t area, inter, uni, pad;
};

// max of avg with the smallest row-major index attaining it and the tie count:
// associative and commutative, so any reduction tree gives the same triple
__device__ __forceinline__ void amax_combine(float& m, uint32_t& idx, uint32_t& cnt, float om, uint32_t oidx,
                                             uint32_t ocnt)
{
    if (om > m) {
        m = om;
        idx = oidx;
        cnt = ocnt;
    } else if (om == m) {
        idx = min(idx, oidx);
        cnt += ocnt;
    }
}

__device__ __forceinline__ void smooth_combine(SmoothPartial& a, const SmoothPartial& b)
{
    a.bmin = fminf(a.bmin, b.bmin);
    a.bmax = fmaxf(a.bmax, b.bmax);
    amax_combine(a.amax, a.idx, a.cnt, b.amax, b.idx, b.cnt);
}

__device__ __forceinline__ SmoothPartial smooth_shfl_xor(const SmoothPartial& a, int off)
{
    SmoothPartial b;
    b.bmin = __shfl_xor(a.bmin, off);
    b.bmax = __shfl_xor(a.bmax, off);
    b.amax = __shfl_xor(a.amax, off);
    b.idx = (uint32_t)__shfl_xor((int)a.idx, off);
    b.cnt = (uint32_t)__shfl_xor((int)a.cnt, off);
    return b;
}

__device__ __forceinline__ SmoothPartial smooth_identity()
{
    return SmoothPartial{INFINITY, -INFINITY, -INFINITY, 0xffffffffu, 0u};
}

// in-image taps of the radius-r window centred at c on an axis of n pixels
__device__ __forceinline__ int taps(int c, int r, int n) { return min(c + r, n - 1) - max(c - r, 0) + 1; }

// The sums of the 29 consecutive values v[k .. k + 28], k = 0..7, as one fixed
// tree shared by the eight windows: pairs, fours, eights, then 16 + 8 + 4 + 1.
// 122 additions where eight 28-step chains take 224, and a tap passes through
// at most 7 rounded additions (4 levels, 3 joins) instead of 28.
__device__ __forceinline__ void window29(const float (&v)[QP_STRIP + 28], float (&out)[QP_STRIP])
{
    float s2[34], s4[32], s8[24];
#pragma unroll
    for (int i = 0; i < 34; ++i) s2[i] = v[i] + v[i + 1];
#pragma unroll
    for (int i = 0; i < 32; ++i) s4[i] = s2[i] + s2[i + 2];
#pragma unroll
    for (int i = 0; i < 24; ++i) s8[i] = s4[i] + s4[i + 4];
#pragma unroll
    for (int k = 0; k < QP_STRIP; ++k) out[k] = (((s8[k] + s8[k + 8]) + s8[k + 16]) + s4[k + 24]) + v[k + 28];
}

// RMAX sizes the LDS; FIXED (the reference's 29 taps, r = RMAX = 14 at compile
// time): windows in registers, summed by window29; else r <= RMAX at run time:
// windows read from LDS and summed in order, 2 r additions each.
template <int RMAX, bool FIXED>
__global__ __launch_bounds__(QP_THREADS) void k_post_smooth(const float* __restrict__ in, int H, int W, int r_rt,
                                                            float* __restrict__ avg, float* __restrict__ blend,
                                                            SmoothPartial* __restrict__ part)
{
    static_assert(!FIXED || RMAX == 14, "the register path is window29");
    constexpr int SHM = QP_TH + 2 * RMAX;
    constexpr int SWP = QP_TW + 2 * RMAX + 1;   // odd strides: a wave's rows (row pass) land on distinct banks
    constexpr int TWP = QP_TW + 1;
    __shared__ float s_in[SHM * SWP];
    __shared__ float s_row[SHM * TWP];
    __shared__ SmoothPartial s_red[QP_WAVES];

    const int r = FIXED ? RMAX : r_rt;
    const int sh = QP_TH + 2 * r;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * QP_TW, y0 = blockIdx.y * QP_TH;
    const size_t pbase = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const float* src = in + pbase;

    // stage one row per wave and step (zeros outside the image).  The pass is bound by the latency of
    // these loads, so a wave issues all of its rows' loads (29 taps: 15 rows, 30 loads) before it stores
    constexpr int QP_BATCH = FIXED ? SHM / QP_WAVES : 12;
    for (int lb = tid >> 6; lb < sh; lb += QP_WAVES * QP_BATCH) {
        const int lane = tid & 63;
        const int gxa = x0 - r + lane, gxb = gxa + 64;
        float va[QP_BATCH], vb[QP_BATCH];
#pragma unroll
        for (int u = 0; u < QP_BATCH; ++u) {
            const int ly = lb + u * QP_WAVES, gy = y0 - r + ly;
            const bool rowin = ly < sh && gy >= 0 && gy < H;
            va[u] = (rowin && gxa >= 0 && gxa < W) ? src[(size_t)gy * W + gxa] : 0.f;
            vb[u] = (rowin && lane < 2 * r && gxb < W) ? src[(size_t)gy * W + gxb] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < QP_BATCH; ++u) {
            const int ly = lb + u * QP_WAVES;
            if (ly < sh) {
                s_in[ly * SWP + lane] = va[u];
                if (lane < 2 * r) s_in[ly * SWP + 64 + lane] = vb[u];
            }
        }
    }
    __syncthreads();

    // row sums: one 8-output strip of one staged row per work item, consecutive lanes on consecutive rows
    for (int w = tid; w < sh * (QP_TW / QP_STRIP); w += QP_THREADS) {
        const int row = w % sh, c0 = (w / sh) * QP_STRIP;
        const float* p = &s_in[row * SWP + c0];
        float* q = &s_row[row * TWP + c0];
        if constexpr (FIXED) {
            float v[QP_STRIP + 2 * RMAX];
#pragma unroll
            for (int j = 0; j < QP_STRIP + 2 * RMAX; ++j) v[j] = p[j];
            float o[QP_STRIP];
            window29(v, o);
#pragma unroll
            for (int k = 0; k < QP_STRIP; ++k) q[k] = o[k];
        } else {
            for (int k = 0; k < QP_STRIP; ++k) {
                float acc = p[k];
                for (int j = 1; j <= 2 * r; ++j) acc += p[k + j];
                q[k] = acc;
            }
        }
    }
    __syncthreads();

    // column sums: lane = column, wave = 8-row strip
    const int lx = tid & 63, ys = (tid >> 6) * QP_STRIP;
    float a[QP_STRIP];
    {
        const float* p = &s_row[ys * TWP + lx];
        if constexpr (FIXED) {
            float v[QP_STRIP + 2 * RMAX];
#pragma unroll
            for (int j = 0; j < QP_STRIP + 2 * RMAX; ++j) v[j] = p[j * TWP];
            window29(v, a);
        } else {
#pragma unroll
            for (int k = 0; k < QP_STRIP; ++k) {
                float acc = p[k * TWP];
                for (int j = 1; j <= 2 * r; ++j) acc += p[(k + j) * TWP];
                a[k] = acc;
            }
        }
    }

    SmoothPartial st = smooth_identity();
    const int gx = x0 + lx;
    if (gx < W) {
        const int nx = taps(gx, r, W);
#pragma unroll
        for (int k = 0; k < QP_STRIP; ++k) {
            const int gy = y0 + ys + k;
            if (gy < H) {
                const float av = a[k] / (float)(taps(gy, r, H) * nx);
                const float v = s_in[(r + ys + k) * SWP + r + lx];
                const float bl = 0.5f * (av + v);
                const size_t o = pbase + (size_t)gy * W + gx;
                if (avg) avg[o] = av;
                if (blend) blend[o] = bl;
                st.bmin = fminf(st.bmin, bl);
                st.bmax = fmaxf(st.bmax, bl);
                // this thread's rows ascend, so a strict > keeps its first pixel
                if (av > st.amax) {
                    st.amax = av;
                    st.idx = (uint32_t)(gy * W + gx);
                    st.cnt = 1;
                } else if (av == st.amax) {
                    st.cnt += 1;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) smooth_combine(st, smooth_shfl_xor(st, off));
    if (lx == 0) s_red[tid >> 6] = st;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < QP_WAVES; ++w) smooth_combine(st, s_red[w]);
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = st;
    }
}

// one workgroup per plane: its tiles' partials, thread-strided then an LDS tree
__global__ __launch_bounds__(QP_THREADS) void k_post_smooth_finish(const SmoothPartial* __restrict__ part, int tiles,
                                                                   float* __restrict__ stats,
                                                                   int64_t* __restrict__ loc)
{
    __shared__ SmoothPartial s_red[QP_THREADS];
    const int tid = threadIdx.x;
    const SmoothPartial* p = part + (size_t)blockIdx.x * tiles;
    SmoothPartial st = smooth_identity();
    for (int t = tid; t < tiles; t += QP_THREADS) smooth_combine(st, p[t]);
    s_red[tid] = st;
    __syncthreads();
    for (int n = QP_THREADS / 2; n >= 1; n >>= 1) {
        if (tid < n) smooth_combine(s_red[tid], s_red[tid + n]);
        __syncthreads();
    }
    if (tid == 0) {
        st = s_red[0];
        stats[(size_t)blockIdx.x * 3 + 0] = st.bmin;
        stats[(size_t)blockIdx.x * 3 + 1] = st.bmax;
        stats[(size_t)blockIdx.x * 3 + 2] = st.amax;
        loc[(size_t)blockIdx.x * 2 + 0] = (int64_t)st.idx;
        loc[(size_t)blockIdx.x * 2 + 1] = (int64_t)st.cnt;
    }
}

// set bits of the (2 s + 1)-wide window starting at staged column lx of a
// staged row held as two ballots (columns 0..127 in four dwords): the two
// dwords the window can touch, funnel-shifted to bit 0
__device__ __forceinline__ int row_count(const uint32_t* w, int lx, uint32_t field)
{
    const uint32_t* p = w + (lx >> 5);
    return __popc(__funnelshift_r(p[0], p[1], lx & 31) & field);
}

template <int SMAX, bool FIXED>
__global__ __launch_bounds__(QP_THREADS) void k_post_mask(const float* __restrict__ blend,
                                                          const float* __restrict__ stats,
                                                          const uint8_t* __restrict__ gt, int n_prompt, int H, int W,
                                                          int s_rt, float thresh, uint8_t* __restrict__ mask,
                                                          MaskPartial* __restrict__ part)
{
    constexpr int SHM = QP_TH + 2 * SMAX;
    __shared__ uint32_t s_bits[SHM][4];
    __shared__ MaskPartial s_red[QP_WAVES];

    const int s = FIXED ? SMAX : s_rt;
    const int sh = QP_TH + 2 * s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * QP_TW, y0 = blockIdx.y * QP_TH;
    const size_t hw = (size_t)H * (size_t)W;
    const float* src = blend + (size_t)blockIdx.z * hw;
    const float mn = stats[(size_t)blockIdx.z * 3 + 0];
    const float den = (stats[(size_t)blockIdx.z * 3 + 1] - mn) + 1e-9f;

    auto raw_of = [&](float b) {
        float o = 2.f * ((b - mn) / den) - 1.f;
        o = o < 0.f ? 0.f : (o > 1.f ? 1.f : o);
        return o > thresh;
    };
    // this thread's own pixels (the masked sum's blend, the annotation), in flight with the staging loads
    const int gx = x0 + lane, ys = wave * QP_STRIP;
    const uint8_t* g = gt ? gt + (size_t)(blockIdx.z % (unsigned)n_prompt) * hw : nullptr;
    float own[QP_STRIP];
    uint8_t ann[QP_STRIP];
#pragma unroll
    for (int k = 0; k < QP_STRIP; ++k) {
        const int gy = y0 + ys + k;
        const bool in = gx < W && gy < H;
        own[k] = in ? src[(size_t)gy * W + gx] : 0.f;
        ann[k] = (in && g) ? g[(size_t)gy * W + gx] : (uint8_t)0;
    }
    // the thresholded tile + s halo as one ballot pair per staged row (zeros outside the image);
    // one row per wave and step, five rows' loads in flight
    constexpr int QP_BATCH = 5;   // (measured: all ten rows at once is 25 % slower)
    for (int lb = wave; lb < sh; lb += QP_WAVES * QP_BATCH) {
        const int gxa = x0 - s + lane, gxb = gxa + 64;
        float va[QP_BATCH], vb[QP_BATCH];
        bool ina[QP_BATCH], inb[QP_BATCH];
#pragma unroll
        for (int u = 0; u < QP_BATCH; ++u) {
            const int ly = lb + u * QP_WAVES, gy = y0 - s + ly;
            const bool rowin = ly < sh && gy >= 0 && gy < H;
            ina[u] = rowin && gxa >= 0 && gxa < W;
            inb[u] = rowin && lane < 2 * s && gxb < W;
            va[u] = ina[u] ? src[(size_t)gy * W + gxa] : 0.f;
            vb[u] = inb[u] ? src[(size_t)gy * W + gxb] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < QP_BATCH; ++u) {
            const int ly = lb + u * QP_WAVES;
            if (ly < sh) {   // the same in every lane of the wave
                const unsigned long long wa = __ballot(ina[u] && raw_of(va[u]));
                const unsigned long long wb = __ballot(inb[u] && raw_of(vb[u]));
                if (lane == 0) {
                    s_bits[ly][0] = (uint32_t)wa;
                    s_bits[ly][1] = (uint32_t)(wa >> 32);
                    s_bits[ly][2] = (uint32_t)wb;
                    s_bits[ly][3] = (uint32_t)(wb >> 32);
                }
            }
        }
    }
    __syncthreads();

    const uint32_t field = (1u << (2 * s + 1)) - 1u;
    int cnt[QP_STRIP];
    if constexpr (FIXED) {
        int c[QP_STRIP + 2 * SMAX];
#pragma unroll
        for (int j = 0; j < QP_STRIP + 2 * SMAX; ++j) c[j] = row_count(s_bits[ys + j], lane, field);
#pragma unroll
        for (int k = 0; k < QP_STRIP; ++k) {
            int acc = 0;
#pragma unroll
            for (int j = 0; j <= 2 * SMAX; ++j) acc += c[k + j];
            cnt[k] = acc;
        }
    } else {
#pragma unroll
        for (int k = 0; k < QP_STRIP; ++k) {
            int acc = 0;
            for (int j = 0; j <= 2 * s; ++j) acc += row_count(s_bits[ys + k + j], lane, field);
            cnt[k] = acc;
        }
    }

    double msum = 0.0;
    uint32_t area = 0, inter = 0, uni = 0;
    if (gx < W) {
        const int nx = taps(gx, s, W);
#pragma unroll
        for (int k = 0; k < QP_STRIP; ++k) {
            const int gy = y0 + ys + k;
            if (gy < H) {
                const bool m = 2 * cnt[k] > taps(gy, s, H) * nx;
                mask[(size_t)blockIdx.z * hw + (size_t)gy * W + gx] = m ? 1 : 0;
                if (m) {
                    msum += (double)own[k];
                    area += 1;
                }
                if (g) {
                    const bool a = ann[k] != 0;
                    inter += (m && a) ? 1 : 0;
                    uni += (m || a) ? 1 : 0;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        msum += __shfl_xor(msum, off);
        area += (uint32_t)__shfl_xor((int)area, off);
        inter += (uint32_t)__shfl_xor((int)inter, off);
        uni += (uint32_t)__shfl_xor((int)uni, off);
    }
    if (lane == 0) s_red[wave] = MaskPartial{msum, area, inter, uni, 0u};
    __syncthreads();
    if (tid == 0) {
        MaskPartial t = s_red[0];
        for (int w = 1; w < QP_WAVES; ++w) {
            t.msum += s_red[w].msum;
            t.area += s_red[w].area;
            t.inter += s_red[w].inter;
            t.uni += s_red[w].uni;
        }
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(QP_THREADS) void k_post_mask_finish(const MaskPartial* __restrict__ part, int tiles,
                                                                 int64_t* __restrict__ counts,
                                                                 float* __restrict__ masked_sum)
{
    __shared__ double s_sum[QP_THREADS];
    __shared__ unsigned long long s_cnt[3][QP_THREADS];
    const int tid = threadIdx.x;
    const MaskPartial* p = part + (size_t)blockIdx.x * tiles;
    double msum = 0.0;
    unsigned long long area = 0, inter = 0, uni = 0;
    for (int t = tid; t < tiles; t += QP_THREADS) {
        msum += p[t].msum;
        area += p[t].area;
        inter += p[t].inter;
        uni += p[t].uni;
    }
    s_sum[tid] = msum;
    s_cnt[0][tid] = area;
    s_cnt[1][tid] = inter;
    s_cnt[2][tid] = uni;
    __syncthreads();
    for (int n = QP_THREADS / 2; n >= 1; n >>= 1) {
        if (tid < n) {
            s_sum[tid] += s_sum[tid + n];
            for (int c = 0; c < 3; ++c) s_cnt[c][tid] += s_cnt[c][tid + n];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int c = 0; c < 3; ++c) counts[(size_t)blockIdx.x * 3 + c] = (int64_t)s_cnt[c][0];
        masked_sum[blockIdx.x] = (float)s_sum[0];
    }
}

inline int tiles_x(int W) { return (W + QP_TW - 1) / QP_TW; }
inline int tiles_y(int H) { return (H + QP_TH - 1) / QP_TH; }

}  // namespace

bool query_post_shape_ok(int planes, int H, int W)
{
    // planes ride in gridDim.z, tile rows in gridDim.y; pixel indices are 32-bit inside a plane
    return planes >= 0 && H >= 0 && W >= 0 && planes <= 65535 && tiles_y(H) <= 65535 &&
           (int64_t)H * W <= (int64_t)0x7fffffff;
}

static size_t smooth_part_bytes(int planes, int H, int W)
{
    const size_t n = (size_t)planes * tiles_x(W) * tiles_y(H) * sizeof(SmoothPartial);
    return (n + 255) & ~(size_t)255;
}

size_t query_post_workspace_bytes(int planes, int H, int W)
{
    if (!query_post_shape_ok(planes, H, W) || planes == 0 || H == 0 || W == 0) return 0;
    return smooth_part_bytes(planes, H, W) + (size_t)planes * tiles_x(W) * tiles_y(H) * sizeof(MaskPartial);
}

hipError_t launch_query_smooth(const float* rel, int planes, int H, int W, int r, float* avg, float* blend,
                               float* stats, int64_t* loc, void* ws, hipStream_t st)
{
    const dim3 grid((unsigned)tiles_x(W), (unsigned)tiles_y(H), (unsigned)planes);
    const int tiles = tiles_x(W) * tiles_y(H);
    SmoothPartial* part = (SmoothPartial*)ws;
    if (r == 14) k_post_smooth<14, true><<<grid, QP_THREADS, 0, st>>>(rel, H, W, r, avg, blend, part);
    else if (r <= 7) k_post_smooth<7, false><<<grid, QP_THREADS, 0, st>>>(rel, H, W, r, avg, blend, part);
    else k_post_smooth<31, false><<<grid, QP_THREADS, 0, st>>>(rel, H, W, r, avg, blend, part);
    k_post_smooth_finish<<<(unsigned)planes, QP_THREADS, 0, st>>>(part, tiles, stats, loc);
    return hipGetLastError();
}

hipError_t launch_query_mask(const float* blend, const float* stats, const uint8_t* gt, int planes, int n_prompt,
                             int H, int W, float thresh, int s, uint8_t* mask, int64_t* counts, float* masked_sum,
                             void* ws, hipStream_t st)
{
    const dim3 grid((unsigned)tiles_x(W), (unsigned)tiles_y(H), (unsigned)planes);
    const int tiles = tiles_x(W) * tiles_y(H);
    MaskPartial* part = (MaskPartial*)((uint8_t*)ws + smooth_part_bytes(planes, H, W));
    if (s == 3)
        k_post_mask<3, true><<<grid, QP_THREADS, 0, st>>>(blend, stats, gt, n_prompt, H, W, s, thresh, mask, part);
    else
        k_post_mask<7, false><<<grid, QP_THREADS, 0, st>>>(blend, stats, gt, n_prompt, H, W, s, thresh, mask, part);
    k_post_mask_finish<<<(unsigned)planes, QP_THREADS, 0, st>>>(part, tiles, counts, masked_sum);
    return hipGetLastError();
}

}  // namespace lsr
