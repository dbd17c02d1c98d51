// photo_loss.hip — the photometric loss of the RGB training step, fused behind
// lsr_photo_loss_forward / lsr_photo_loss_backward.  Replaces, per iteration
// (train.py:170-173, utils/loss_utils.py:18-71):
//   Ll1  = l1_loss(image, gt)                       mean |x - y|
//   ssim = ssim(image, gt)                          mean of the SSIM map, 11x11 Gaussian window
//   loss = (1 - lambda) Ll1 + lambda (1 - ssim)
// which torch runs as five depthwise 11x11 conv2d calls and about fifteen
// elementwise passes over (3, H, W) tensors, and again in reverse under autograd.
//
// Per plane and pixel, with cv the windowed sum (11 taps, sigma 1.5, applied
// separably, zero padding of 5):
//   mu1 = cv(x), mu2 = cv(y), e11 = cv(x^2), e22 = cv(y^2), e12 = cv(xy)
//   A = 2 mu1 mu2 + C1            B = 2 (e12 - mu1 mu2) + C2
//   C = mu1^2 + mu2^2 + C1        D = (e11 - mu1^2) + (e22 - mu2^2) + C2
//   m = A B / (C D)
// The forward writes the two means and, for the backward, the total
// derivatives of m per pixel (the sigma terms expanded):
//   dmu  = 2 mu2 (B - A) / (C D) - 2 mu1 m / C + 2 mu1 m / D
//   de11 = -m / D
//   de12 = 2 A / (C D)
// The window is symmetric and the padding zero, so the adjoint of cv is cv
// over the partial maps taken as zero outside the image; the backward is a
// gather (no atomics):
//   dL/dx_q = g_l1 / N sign(x_q - y_q) + g_ssim / N (cv(dmu) + 2 x_q cv(de11) + y_q cv(de12))[q]
//
// One 256-thread workgroup per (plane, 64 x 16 tile): the inputs with their
// 5-pixel halo are staged in LDS (rows of 80 floats starting 8 columns left of
// the tile, so the body moves as aligned 16-B vectors), the horizontal pass
// leaves 26 rows x 64 columns per quantity in LDS, the vertical pass reads
// columns with consecutive lanes.  Every tap sum is an fmaf chain in tap order.
// The loss sums leave each workgroup as two doubles in its workspace slot; one
// workgroup adds the slots in a fixed order (bit-reproducible means).
#include "lsr_internal.h"

#include <algorithm>

namespace lsr {

#define PL_TW 64                 // tile width
#define PL_TH 16                 // tile height
#define PL_R 5                   // window radius
#define PL_ROWS (PL_TH + 2 * PL_R)   // staged rows
#define PL_SW 80                 // staged row: image columns x0 - 8 .. x0 + 71
#define PL_OFF 3                 // staged column of the first tap of tile column 0 (8 - PL_R)
#define PL_MAX_BLOCKS 8192       // grid cap, ~10 rounds of the resident workgroups; tiles above it are strided over
#define PL_C1 1e-4f
#define PL_C2 9e-4f

namespace {

struct PLTile {
    int plane_off;   // element offset of the plane (planes H W < 2^31)
    int x0, y0;
};

__device__ __forceinline__ PLTile pl_tile(uint32_t tile, int ntx, int nty, int H, int W)
{
    const uint32_t per_plane = (uint32_t)ntx * nty;
    const uint32_t plane = tile / per_plane, r = tile % per_plane;
    PLTile t;
    t.plane_off = (int)(plane * (uint32_t)(H * W));
    t.x0 = (int)(r % ntx) * PL_TW;
    t.y0 = (int)(r / ntx) * PL_TH;
    return t;
}

// Stage rows y0 - 5 .. y0 + 20, columns x0 - 8 .. x0 + 71 of a plane, zero
// outside the image.  vec: W % 4 == 0 and a 16-B aligned base, so an aligned
// group of four columns lies wholly inside or outside the image.
__device__ __forceinline__ void pl_stage(const float* __restrict__ plane, int H, int W, int x0, int y0, bool vec,
                                         float* __restrict__ s)
{
    if (vec) {
        for (int i = threadIdx.x; i < PL_ROWS * (PL_SW / 4); i += 256) {
            const int r = i / (PL_SW / 4), c = (i % (PL_SW / 4)) * 4;
            const int gy = y0 - PL_R + r, gx = x0 - 8 + c;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(plane + gy * W + gx);
            *reinterpret_cast<float4*>(s + r * PL_SW + c) = v;
        }
    } else {
        for (int i = threadIdx.x; i < PL_ROWS * PL_SW; i += 256) {
            const int r = i / PL_SW, c = i % PL_SW;
            const int gy = y0 - PL_R + r, gx = x0 - 8 + c;
            s[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? plane[gy * W + gx] : 0.f;
        }
    }
}

__device__ __forceinline__ void pl_load20(const float* __restrict__ s, float (&v)[20])
{
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const float4 a = *reinterpret_cast<const float4*>(s + 4 * j);
        v[4 * j] = a.x, v[4 * j + 1] = a.y, v[4 * j + 2] = a.z, v[4 * j + 3] = a.w;
    }
}

// four adjacent outputs of the horizontal pass from the 20 staged values under them
__device__ __forceinline__ float4 pl_hsum(const float (&v)[20], const PhotoTaps& tp)
{
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) a = fmaf(tp.w[k], v[PL_OFF + j + k], a);
        o[j] = a;
    }
    return make_float4(o[0], o[1], o[2], o[3]);
}

// vertical pass: the four output rows 4 ty .. 4 ty + 3 of column tx from the
// 14 rows of the horizontal pass under them
__device__ __forceinline__ void pl_vsum(const float* __restrict__ h, int tx, int ty, const PhotoTaps& tp,
                                        float (&o)[4])
{
    float v[14];
#pragma unroll
    for (int r = 0; r < 14; r++) v[r] = h[(4 * ty + r) * PL_TW + tx];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) a = fmaf(tp.w[k], v[j + k], a);
        o[j] = a;
    }
}

__device__ __forceinline__ double pl_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

}  // namespace

__global__ void __launch_bounds__(256) k_photo_fwd(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                   int W, int ntx, int nty, uint32_t ntiles, bool vec,
                                                   PhotoTaps tp, float* __restrict__ partials, size_t N,
                                                   double* __restrict__ slots)
{
    __shared__ __attribute__((aligned(16))) float sIn[2][PL_ROWS * PL_SW];
    __shared__ __attribute__((aligned(16))) float sH[5][PL_ROWS * PL_TW];
    __shared__ double sRed[2][4];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    double acc_l1 = 0.0, acc_m = 0.0;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const PLTile t = pl_tile(tile, ntx, nty, H, W);
        pl_stage(x + t.plane_off, H, W, t.x0, t.y0, vec, sIn[0]);
        pl_stage(y + t.plane_off, H, W, t.x0, t.y0, vec, sIn[1]);
        __syncthreads();
        for (int i = threadIdx.x; i < PL_ROWS * (PL_TW / 4); i += 256) {
            const int r = i / (PL_TW / 4), c = (i % (PL_TW / 4)) * 4;
            float vx[20], vy[20], p[20];
            pl_load20(sIn[0] + r * PL_SW + c, vx);
            pl_load20(sIn[1] + r * PL_SW + c, vy);
            float* o = &sH[0][r * PL_TW + c];
            *reinterpret_cast<float4*>(o) = pl_hsum(vx, tp);
            *reinterpret_cast<float4*>(o + PL_ROWS * PL_TW) = pl_hsum(vy, tp);
#pragma unroll
            for (int j = 0; j < 20; j++) p[j] = vx[j] * vx[j];
            *reinterpret_cast<float4*>(o + 2 * PL_ROWS * PL_TW) = pl_hsum(p, tp);
#pragma unroll
            for (int j = 0; j < 20; j++) p[j] = vy[j] * vy[j];
            *reinterpret_cast<float4*>(o + 3 * PL_ROWS * PL_TW) = pl_hsum(p, tp);
#pragma unroll
            for (int j = 0; j < 20; j++) p[j] = vx[j] * vy[j];
            *reinterpret_cast<float4*>(o + 4 * PL_ROWS * PL_TW) = pl_hsum(p, tp);
        }
        __syncthreads();
        float mu1[4], mu2[4], e11[4], e22[4], e12[4];
        pl_vsum(sH[0], tx, ty, tp, mu1);
        pl_vsum(sH[1], tx, ty, tp, mu2);
        pl_vsum(sH[2], tx, ty, tp, e11);
        pl_vsum(sH[3], tx, ty, tp, e22);
        pl_vsum(sH[4], tx, ty, tp, e12);
        float l1 = 0.f, ms = 0.f;
        const int px = t.x0 + tx;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int py = t.y0 + 4 * ty + j;
            if (px >= W || py >= H) continue;
            const int sidx = (4 * ty + j + PL_R) * PL_SW + 8 + tx;
            l1 += fabsf(sIn[0][sidx] - sIn[1][sidx]);
            const float m12 = mu1[j] * mu2[j];
            const float A = fmaf(2.f, m12, PL_C1);
            const float B = fmaf(2.f, fmaf(-mu1[j], mu2[j], e12[j]), PL_C2);
            const float C = fmaf(mu1[j], mu1[j], fmaf(mu2[j], mu2[j], PL_C1));
            const float D = fmaf(-mu1[j], mu1[j], e11[j]) + fmaf(-mu2[j], mu2[j], e22[j]) + PL_C2;
            const float rC = 1.f / C, rD = 1.f / D;
            const float rCD = rC * rD;
            const float m = A * B * rCD;
            ms += m;
            if (partials) {
                const size_t q = (size_t)t.plane_off + (size_t)py * W + px;
                partials[q] = 2.f * mu2[j] * (B - A) * rCD + 2.f * mu1[j] * m * (rD - rC);
                partials[N + q] = -m * rD;
                partials[2 * N + q] = 2.f * A * rCD;
            }
        }
        acc_l1 += (double)l1;
        acc_m += (double)ms;
        __syncthreads();   // the staged tiles are rewritten by the next iteration
    }
    acc_l1 = pl_wave_sum(acc_l1);
    acc_m = pl_wave_sum(acc_m);
    if (tx == 0) sRed[0][ty] = acc_l1, sRed[1][ty] = acc_m;
    __syncthreads();
    if (threadIdx.x < 2) {
        const double* r = sRed[threadIdx.x];
        slots[2 * (size_t)blockIdx.x + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// out[0] = sum of the l1 slots / N, out[1] = sum of the ssim slots / N: each
// thread adds its slots in index order, then a fixed tree
__global__ void __launch_bounds__(256) k_photo_total(const double* __restrict__ slots, int n, size_t N,
                                                     float* __restrict__ out)
{
    __shared__ double sh[2][256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += slots[2 * (size_t)i], b += slots[2 * (size_t)i + 1];
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + m];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) out[threadIdx.x] = (float)(sh[threadIdx.x][0] / (double)N);
}

__global__ void __launch_bounds__(256) k_photo_bwd(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                   int W, int ntx, int nty, uint32_t ntiles, bool vec,
                                                   PhotoTaps tp, const float* __restrict__ partials, size_t N,
                                                   const float* __restrict__ g, float* __restrict__ gx)
{
    __shared__ __attribute__((aligned(16))) float sIn[3][PL_ROWS * PL_SW];
    __shared__ __attribute__((aligned(16))) float sH[3][PL_ROWS * PL_TW];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const float g_l1 = g[0] / (float)N, g_ssim = g[1] / (float)N;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const PLTile t = pl_tile(tile, ntx, nty, H, W);
#pragma unroll
        for (int k = 0; k < 3; k++) pl_stage(partials + k * N + t.plane_off, H, W, t.x0, t.y0, vec, sIn[k]);
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * PL_ROWS * (PL_TW / 4); i += 256) {
            const int k = i / (PL_ROWS * (PL_TW / 4)), ri = i % (PL_ROWS * (PL_TW / 4));
            const int r = ri / (PL_TW / 4), c = (ri % (PL_TW / 4)) * 4;
            float v[20];
            pl_load20(sIn[k] + r * PL_SW + c, v);
            *reinterpret_cast<float4*>(&sH[k][r * PL_TW + c]) = pl_hsum(v, tp);
        }
        __syncthreads();
        float s_mu[4], s_e11[4], s_e12[4];
        pl_vsum(sH[0], tx, ty, tp, s_mu);
        pl_vsum(sH[1], tx, ty, tp, s_e11);
        pl_vsum(sH[2], tx, ty, tp, s_e12);
        const int px = t.x0 + tx;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int py = t.y0 + 4 * ty + j;
            if (px >= W || py >= H) continue;
            const int q = t.plane_off + py * W + px;
            const float xv = x[q], yv = y[q];
            const float d = xv - yv;
            const float sgn = (float)(d > 0.f) - (float)(d < 0.f);
            const float ds = fmaf(2.f * xv, s_e11[j], fmaf(yv, s_e12[j], s_mu[j]));
            gx[q] = fmaf(g_l1, sgn, g_ssim * ds);
        }
        __syncthreads();
    }
}

static uint32_t photo_tiles(int planes, int H, int W, int* ntx, int* nty)
{
    *ntx = (W + PL_TW - 1) / PL_TW;
    *nty = (H + PL_TH - 1) / PL_TH;
    return (uint32_t)((int64_t)planes * *ntx * *nty);   // <= planes H W < 2^31
}

static bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

size_t photo_loss_workspace_bytes(int planes, int H, int W)
{
    int ntx, nty;
    const uint32_t nt = photo_tiles(planes, H, W, &ntx, &nty);
    return 2 * sizeof(double) * (size_t)std::min<uint32_t>(nt, PL_MAX_BLOCKS);
}

hipError_t launch_photo_loss_fwd(const float* x, const float* y, int planes, int H, int W,
                                 const PhotoTaps& tp, float* out, float* partials, void* ws, hipStream_t st)
{
    int ntx, nty;
    const uint32_t nt = photo_tiles(planes, H, W, &ntx, &nty);
    const int nb = (int)std::min<uint32_t>(nt, PL_MAX_BLOCKS);
    const size_t N = (size_t)planes * H * W;
    const bool vec = (W % 4) == 0 && aligned16(x) && aligned16(y);
    k_photo_fwd<<<nb, 256, 0, st>>>(x, y, H, W, ntx, nty, nt, vec, tp, partials, N, (double*)ws);
    k_photo_total<<<1, 256, 0, st>>>((const double*)ws, nb, N, out);
    return hipGetLastError();
}

hipError_t launch_photo_loss_bwd(const float* x, const float* y, int planes, int H, int W,
                                 const PhotoTaps& tp, const float* partials, const float* g, float* gx,
                                 hipStream_t st)
{
    int ntx, nty;
    const uint32_t nt = photo_tiles(planes, H, W, &ntx, &nty);
    const int nb = (int)std::min<uint32_t>(nt, PL_MAX_BLOCKS);
    const size_t N = (size_t)planes * H * W;
    const bool vec = (W % 4) == 0 && aligned16(partials);
    k_photo_bwd<<<nb, 256, 0, st>>>(x, y, H, W, ntx, nty, nt, vec, tp, partials, N, g, gx);
    return hipGetLastError();
}

}  // namespace lsr
