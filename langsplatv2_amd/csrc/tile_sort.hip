// tile_sort.hip — per-tile depth sort of the binning's buckets (A.2): the
// bucket's unique u64 keys (depth bits << 32 | id) in, the sorted ids out.
// One wave per tile with the keys in registers (k_tile_sort_wave, n <= 1024);
// a workgroup in LDS for n <= 8192, chunked LDS + global merge above.  The
// size classes and their lists: tile_sort.h.
#include "tile_sort.h"

#include <algorithm>

namespace lsr {

// Classification pass for the global-atomic binning path (the privatised path
// classifies inside k_bin_table).  cls_cnt must be zero.
__global__ void __launch_bounds__(256) k_tile_classify(int T, const uint32_t* __restrict__ tile_start,
                                                       uint32_t* __restrict__ cls_cnt, uint32_t* __restrict__ cls_list)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = t < T ? (int)(tile_start[t + 1] - tile_start[t]) : 0;
    tile_class_append(t < T, t, n, T, cls_cnt, cls_list);
}

// ------------------------------------------------------------ tile sort ---
// Ascending flip-bitonic network over n keys with virtual +inf padding to the
// next power of two: every compare-exchange puts the minimum at the lower
// index, so pairs whose upper index is >= n are no-ops and are skipped.
#define SORT_BLOCK 256
#define SORT_CHUNK 4096

__device__ __forceinline__ void ce(uint64_t* a, int i, int l)
{
    uint64_t x = a[i], y = a[l];
    if (x > y) { a[i] = y; a[l] = x; }
}

// Full network for k = 2..SORT_CHUNK over a[0, n) (n <= SORT_CHUNK), in LDS.
__device__ void bitonic_lds(uint64_t* a, int n)
{
    for (int k = 2; k <= SORT_CHUNK; k <<= 1) {
        const int hk = k >> 1;
        for (int p = threadIdx.x; p < SORT_CHUNK / 2; p += SORT_BLOCK) {
            const int blk = p / hk, off = p % hk;
            const int i = blk * k + off, l = blk * k + k - 1 - off;
            if (l < n) ce(a, i, l);
        }
        __syncthreads();
        for (int j = k >> 2; j >= 1; j >>= 1) {
            for (int p = threadIdx.x; p < SORT_CHUNK / 2; p += SORT_BLOCK) {
                const int i = (p / j) * 2 * j + (p % j), l = i + j;
                if (l < n) ce(a, i, l);
            }
            __syncthreads();
        }
    }
}

// Half-cleaner steps j = jmax..1 over a[0, n) in LDS (n <= chunk).
__device__ void halfclean_lds(uint64_t* a, int n, int chunk, int jmax)
{
    for (int j = jmax; j >= 1; j >>= 1) {
        for (int p = threadIdx.x; p < chunk / 2; p += SORT_BLOCK) {
            const int i = (p / j) * 2 * j + (p % j), l = i + j;
            if (l < n) ce(a, i, l);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int next_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// Tiles of class 4 (n > 8192 = 2 SORT_CHUNK): one workgroup per tile
// (grid-stride over the class list), chunk-local bitonic stages in LDS,
// cross-chunk stages in global memory (the workgroup owns the tile;
// __syncthreads orders its passes).
__device__ void tile_sort_big(int t, const uint32_t* __restrict__ tile_start, uint64_t* __restrict__ keys,
                              uint32_t* __restrict__ point_list, uint64_t* buf)
{
    const uint32_t s0 = tile_start[t], s1 = tile_start[t + 1];
    const int n = (int)(s1 - s0);
    uint64_t* g = keys + s0;
    const int n2 = next_pow2(n);
    const int nch = (n + SORT_CHUNK - 1) / SORT_CHUNK;
    for (int ch = 0; ch < nch; ch++) {
        const int cb = ch * SORT_CHUNK, cn = min(SORT_CHUNK, n - cb);
        for (int k = threadIdx.x; k < cn; k += SORT_BLOCK) buf[k] = g[cb + k];
        __syncthreads();
        bitonic_lds(buf, cn);
        for (int k = threadIdx.x; k < cn; k += SORT_BLOCK) g[cb + k] = buf[k];
        __syncthreads();
    }
    for (int k = 2 * SORT_CHUNK; k <= n2; k <<= 1) {
        const int hk = k >> 1;
        for (int p = threadIdx.x; p < n2 / 2; p += SORT_BLOCK) {
            const int blk = p / hk, off = p % hk;
            const int i = blk * k + off, l = blk * k + k - 1 - off;
            if (l < n) ce(g, i, l);
        }
        __syncthreads();
        for (int j = k >> 2; j >= SORT_CHUNK; j >>= 1) {
            for (int p = threadIdx.x; p < n2 / 2; p += SORT_BLOCK) {
                const int i = (p / j) * 2 * j + (p % j), l = i + j;
                if (l < n) ce(g, i, l);
            }
            __syncthreads();
        }
        for (int ch = 0; ch < nch; ch++) {
            const int cb = ch * SORT_CHUNK, cn = min(SORT_CHUNK, n - cb);
            for (int q = threadIdx.x; q < cn; q += SORT_BLOCK) buf[q] = g[cb + q];
            __syncthreads();
            halfclean_lds(buf, cn, SORT_CHUNK, SORT_CHUNK / 2);
            for (int q = threadIdx.x; q < cn; q += SORT_BLOCK) g[cb + q] = buf[q];
            __syncthreads();
        }
    }
    for (int k = threadIdx.x; k < n; k += SORT_BLOCK) point_list[s0 + k] = (uint32_t)g[k];
    __syncthreads();
}

__global__ void __launch_bounds__(SORT_BLOCK) k_tile_sort_big(int T, const uint32_t* __restrict__ tile_start,
                                                              uint64_t* __restrict__ keys,
                                                              uint32_t* __restrict__ point_list,
                                                              const uint32_t* __restrict__ cls_cnt,
                                                              const uint32_t* __restrict__ cls_list)
{
    __shared__ uint64_t buf[SORT_CHUNK];
    const uint32_t cnt = cls_cnt[4];
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x)
        tile_sort_big((int)cls_list[(size_t)4 * T + i], tile_start, keys, point_list, buf);
}

// Wave-level register bitonic sort of a full run of 64*KPL keys (the 4-wave
// block sort's per-wave runs): lane l holds elements [l*KPL, l*KPL + KPL)
// (padding = UINT64_MAX).  Steps whose partner distance j < KPL run inside the
// lane's registers; the others pair lane l with lane l ^ (j / KPL) through
// lane exchanges.  No LDS, no barriers.  (The one-wave tile sort has its own
// network, sized by the key count: wave_sort_tile below.)
//
// xor_lane_u32 (the register-path lane exchange) lives in lsr_device.h, where
// tests/micro/micro_checks.hip checks it against __shfl_xor on the GPU.
template <int M>
__device__ __forceinline__ uint64_t xor_lane_u64(uint64_t v)
{
    const uint32_t lo = xor_lane_u32<M>((uint32_t)v);
    const uint32_t hi = xor_lane_u32<M>((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <int KPL, int K, int J>
__device__ __forceinline__ void wave_sort_xstep(uint64_t (&v)[KPL])
{
    constexpr int M = J / KPL;
    const int lane = threadIdx.x & 63;
    // K >= 2J >= 2 KPL: the direction bit of element lane*KPL + r is the
    // lane's alone, so one flag serves all KPL elements
    const bool take_min = ((lane & M) == 0) == (((lane * KPL) & K) == 0);
    // every partner first, then every select (keep the own value iff it is
    // the wanted one): the lane exchanges (DPP / permlane) read registers the
    // previous step wrote long before, so no hazard wait states sit between a
    // select and the exchange that needs it
    uint64_t o[KPL];
#pragma unroll
    for (int r = 0; r < KPL; r++) o[r] = xor_lane_u64<M>(v[r]);
#pragma unroll
    for (int r = 0; r < KPL; r++) v[r] = ((v[r] < o[r]) == take_min) ? v[r] : o[r];
}

template <int KPL, int K, int J>
__device__ __forceinline__ void wave_sort_steps(uint64_t (&v)[KPL])
{
    if constexpr (J >= 1) {
        if constexpr (J < KPL) {
            const int lane = threadIdx.x & 63;
            // direction of element lane*KPL + r: from r alone while K < KPL
            // (compile time), from the lane alone once K >= KPL (r < KPL <= K
            // never reaches bit K): one compare + one mask XOR per pair
            const bool desc_lane = ((lane * KPL) & K) != 0;
#pragma unroll
            for (int r = 0; r < KPL; r++) {
                if (r & J) continue;
                const uint64_t a = v[r], b = v[r | J];
                bool sw;
                if constexpr (K < KPL) sw = (r & K) ? (a < b) : (a > b);
                else sw = (a > b) != desc_lane;
                v[r] = sw ? b : a;
                v[r | J] = sw ? a : b;
            }
        } else {
            wave_sort_xstep<KPL, K, J>(v);
        }
        wave_sort_steps<KPL, K, J / 2>(v);
    }
}

template <int KPL, int K>
__device__ __forceinline__ void wave_sort_stages(uint64_t (&v)[KPL])
{
    if constexpr (K <= 64 * KPL) {
        wave_sort_steps<KPL, K, K / 2>(v);
        wave_sort_stages<KPL, 2 * K>(v);
    }
}

// The one-wave tile sort (class 0) sizes its network by the tile's key count:
// KPL = ceil(n / 64) keys per lane, not a power of two (the power-of-two network
// it replaces ran 1024 slots for cfg3's 487..715 keys).  Lane l holds elements
// [l*KPL, l*KPL + KPL), +inf from n up.  A merge sort whose runs are lanes:
//  - every lane sorts its KPL registers (Batcher's odd-even merge sort, which
//    exists for every length: 32 compare-exchanges at KPL = 10, 63 at 16);
//  - for m = 2, 4 .. 64 lanes: the flip pairs element (l, r) with
//    (l ^ (m - 1), KPL - 1 - r), the minimum to the lower lane, which leaves
//    both halves bitonic and the lower one below the upper; half-cleaners at
//    lane distances m/4 .. 1 (every register against the same register of
//    lane l ^ d) then leave every lane a bitonic KPL keys that lie between
//    its neighbours', and the lane's own sort finishes the stage.
// The flip and the half-cleaner hold for runs of any equal length, so nothing
// is padded to a power of two.  21 lane-exchange steps in all (the log2 m of
// every stage), each over KPL registers, with every partner fetched before
// every select as in wave_sort_xstep.  Same keys, total order: the output is
// the full network's.
template <int KPL>
__device__ __forceinline__ void lane_sort_regs(uint64_t (&v)[KPL])
{
    // odd-even merge sort over v[0, KPL), every index a compile-time constant
#pragma unroll
    for (int p = 1; p < KPL; p *= 2) {
#pragma unroll
        for (int k = p; k >= 1; k /= 2) {
#pragma unroll
            for (int j = k % p; j + k < KPL; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < k; i++) {
                    const int a = i + j, b = i + j + k;
                    if (b >= KPL || a / (2 * p) != b / (2 * p)) continue;
                    const uint64_t x = v[a], y = v[b];
                    const bool sw = x > y;
                    v[a] = sw ? y : x;
                    v[b] = sw ? x : y;
                }
            }
        }
    }
}

// One lane-exchange step: register r against register (FLIP ? KPL - 1 - r : r)
// of lane l ^ M; the lane whose bit LOW is clear keeps the minimum.
template <int KPL, int M, int LOW, bool FLIP>
__device__ __forceinline__ void wsort_xstep(uint64_t (&v)[KPL])
{
    const int lane = threadIdx.x & 63;
    const bool take_min = (lane & LOW) == 0;
    uint64_t o[KPL];
#pragma unroll
    for (int r = 0; r < KPL; r++) o[r] = xor_lane_u64<M>(v[FLIP ? KPL - 1 - r : r]);
#pragma unroll
    for (int r = 0; r < KPL; r++) v[r] = ((v[r] < o[r]) == take_min) ? v[r] : o[r];
}

template <int KPL, int D>
__device__ __forceinline__ void wsort_halfclean(uint64_t (&v)[KPL])
{
    if constexpr (D >= 1) {
        wsort_xstep<KPL, D, D, false>(v);
        wsort_halfclean<KPL, D / 2>(v);
    }
}

template <int KPL, int M>
__device__ __forceinline__ void wsort_merge_lanes(uint64_t (&v)[KPL])
{
    if constexpr (M <= 64) {
        wsort_xstep<KPL, M - 1, M / 2, true>(v);
        wsort_halfclean<KPL, M / 4>(v);
        lane_sort_regs<KPL>(v);
        wsort_merge_lanes<KPL, 2 * M>(v);
    }
}

// n <= 64 KPL keys of one tile, sorted by one wave.
template <int KPL>
__device__ __forceinline__ void wave_sort_tile(const uint64_t* __restrict__ g, uint32_t* __restrict__ out, int n)
{
    const int lane = threadIdx.x & 63;
    uint64_t v[KPL];
#pragma unroll
    for (int r = 0; r < KPL; r++) {
        const int e = lane * KPL + r;
        v[r] = e < n ? g[e] : ~0ull;
    }
    lane_sort_regs<KPL>(v);
    wsort_merge_lanes<KPL, 2>(v);
#pragma unroll
    for (int r = 0; r < KPL; r++) {
        const int e = lane * KPL + r;
        if (e < n) out[e] = (uint32_t)v[r];
    }
}

// LDS slot of logical element e of a block sort: one u64 of padding every 16
// keys, so the lane-major run reads (lane stride KPL*8 bytes) spread over
// the banks instead of piling onto a few.
__device__ __forceinline__ int lpad(int e) { return e + (e >> 4); }

// Merge-path co-rank: how many of the first d outputs of merge(A, B) come
// from A, A = lds[a0, a0+na), B = lds[b0, b0+nb) (logical indices; keys are
// unique, so ties never occur).
__device__ __forceinline__ int merge_corank(const uint64_t* lds, int a0, int na, int b0, int nb, int d)
{
    int lo = max(0, d - nb), hi = min(d, na);
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (lds[lpad(a0 + m)] < lds[lpad(b0 + d - 1 - m)]) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// KPL consecutive outputs of merge(A, B) starting at output d, into v.
template <int KPL>
__device__ __forceinline__ void merge_run(const uint64_t* lds, int a0, int na, int b0, int nb, int d,
                                          uint64_t (&v)[KPL])
{
    int i = merge_corank(lds, a0, na, b0, nb, d), j = d - i;
    uint64_t a = i < na ? lds[lpad(a0 + i)] : ~0ull, b = j < nb ? lds[lpad(b0 + j)] : ~0ull;
#pragma unroll
    for (int k = 0; k < KPL; k++) {
        const bool ta = a < b;
        v[k] = ta ? a : b;
        i += ta ? 1 : 0;
        j += ta ? 0 : 1;
        const bool ok = ta ? (i < na) : (j < nb);
        const uint64_t nx = ok ? lds[lpad(ta ? a0 + i : b0 + j)] : ~0ull;
        a = ta ? nx : a;
        b = ta ? b : nx;
    }
}

// One 4-wave workgroup per tile of 128*KPL < n <= 256*KPL keys.  The bucket
// is staged into LDS with coalesced loads (+inf padding), each wave sorts a
// 64*KPL run in registers (the wave bitonic network above), two merge-path
// rounds (every thread producing KPL consecutive outputs after a binary
// co-rank search) finish the order, and the ids leave through LDS with
// coalesced stores.
template <int KPL>
__device__ __forceinline__ void block_sort_tile(const uint64_t* __restrict__ g, uint32_t* __restrict__ out, int n,
                                                uint64_t* lds)
{
    constexpr int R = 64 * KPL;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // batches of 8 loads in flight per thread (a full unroll would hold all
    // 4*KPL keys in VGPRs and collapse occupancy)
#pragma unroll 1
    for (int k0 = 0; k0 < 4 * KPL; k0 += 8) {
        uint64_t x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int e = (k0 + k) * 256 + tid;
            x[k] = e < n ? g[e] : ~0ull;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) lds[lpad((k0 + k) * 256 + tid)] = x[k];
    }
    __syncthreads();
    uint64_t v[KPL];
#pragma unroll
    for (int r = 0; r < KPL; r++) v[r] = lds[lpad(w * R + lane * KPL + r)];
    wave_sort_stages<KPL, 2>(v);
#pragma unroll
    for (int r = 0; r < KPL; r++) lds[lpad(w * R + lane * KPL + r)] = v[r];
    __syncthreads();
    {
        const int p0 = (tid >> 7) * 2 * R, d = (tid & 127) * KPL;
        merge_run<KPL>(lds, p0, R, p0 + R, R, d, v);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KPL; k++) lds[lpad(p0 + d + k)] = v[k];
    }
    __syncthreads();
    const int d = tid * KPL;
    merge_run<KPL>(lds, 0, 2 * R, 2 * R, 2 * R, d, v);
    __syncthreads();
    uint32_t* l32 = (uint32_t*)lds;
#pragma unroll
    for (int k = 0; k < KPL; k++) l32[d + k + ((d + k) >> 5)] = (uint32_t)v[k];
    __syncthreads();
#pragma unroll 8
    for (int e = tid; e < n; e += 256) out[e] = l32[e + (e >> 5)];
    __syncthreads();
}

// Class c = 1..3 (KPL = 4 << c): one workgroup per listed tile.
template <int KPL>
__global__ void __launch_bounds__(256) k_tile_sort_blk(int T, const uint32_t* __restrict__ tile_start,
                                                       const uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ point_list,
                                                       const uint32_t* __restrict__ cls_cnt,
                                                       const uint32_t* __restrict__ cls_list, int cls)
{
    __shared__ uint64_t lds[(4 * 64 * KPL) * 17 / 16];
    const uint32_t cnt = cls_cnt[cls];
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        const int t = (int)cls_list[(size_t)cls * T + i];
        const uint32_t s0 = tile_start[t];
        block_sort_tile<KPL>(keys + s0, point_list + s0, (int)(tile_start[t + 1] - s0), lds);
    }
}

// Class 0 (n <= LSR_SORT_WAVE_MAX): one wave per listed tile, four per workgroup.
// (capped at the 128 VGPRs of 4 waves per SIMD, the occupancy of the power-of-two
// network it replaces: uncapped the scheduler takes 136)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_tile_sort_wave(int T, const uint32_t* __restrict__ tile_start,
                                                        const uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ point_list,
                                                        const uint32_t* __restrict__ cls_cnt,
                                                        const uint32_t* __restrict__ cls_list)
{
    const uint32_t cnt = cls_cnt[0];
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt; i += gridDim.x * 4) {
        const int t = (int)cls_list[i];
        const uint32_t s0 = tile_start[t];
        const int n = (int)(tile_start[t + 1] - s0);
        const uint64_t* g = keys + s0;
        uint32_t* o = point_list + s0;
        // keys per lane: every count up to 4, even counts above (the odd ones from 5
        // up spill at the 128 VGPRs of 4 waves per SIMD)
        if (n == 1) {
            if ((threadIdx.x & 63) == 0) o[0] = (uint32_t)g[0];
            continue;
        }
        int kpl = (n + 63) >> 6;
        if (kpl > 4) kpl = (kpl + 1) & ~1;
        switch (kpl) {
        case 1: wave_sort_tile<1>(g, o, n); break;
        case 2: wave_sort_tile<2>(g, o, n); break;
        case 3: wave_sort_tile<3>(g, o, n); break;
        case 4: wave_sort_tile<4>(g, o, n); break;
        case 6: wave_sort_tile<6>(g, o, n); break;
        case 8: wave_sort_tile<8>(g, o, n); break;
        case 10: wave_sort_tile<10>(g, o, n); break;
        case 12: wave_sort_tile<12>(g, o, n); break;
        case 14: wave_sort_tile<14>(g, o, n); break;
        default: wave_sort_tile<16>(g, o, n); break;
        }
    }
}

// host_cnt: lsr_internal.h.
hipError_t launch_tile_sort(int T, const BinWs& ws, uint64_t* keys, uint32_t* point_list, const uint32_t* host_cnt,
                            hipStream_t st)
{
    if (T == 0) return hipSuccess;
    uint32_t cnt[SORT_NCLS];
    if (host_cnt) {
        for (int k = 0; k < SORT_NCLS; k++) cnt[k] = host_cnt[k];
    } else {
        (void)hipMemsetAsync(ws.cls_cnt, 0, SORT_NCLS * 4, st);
        k_tile_classify<<<(T + 255) / 256, 256, 0, st>>>(T, ws.tile_start, ws.cls_cnt, ws.cls_list);
        // persistent grids: enough workgroups to fill the chip, or the tiles
        // (class 0: four tiles per workgroup)
        const uint32_t fill[SORT_NCLS] = {256 * 8 * 4, 256 * 8, 256 * 4, 256 * 2, 256 * 2};
        for (int k = 0; k < SORT_NCLS; k++) cnt[k] = std::min<uint32_t>((uint32_t)T, fill[k]);
    }
    const uint32_t* ts = ws.tile_start;
    const uint32_t* cc = ws.cls_cnt;
    const uint32_t* cl = ws.cls_list;
    if (cnt[0]) k_tile_sort_wave<<<(cnt[0] + 3) / 4, 256, 0, st>>>(T, ts, keys, point_list, cc, cl);
    if (cnt[1]) k_tile_sort_blk<8><<<cnt[1], 256, 0, st>>>(T, ts, keys, point_list, cc, cl, 1);
    if (cnt[2]) k_tile_sort_blk<16><<<cnt[2], 256, 0, st>>>(T, ts, keys, point_list, cc, cl, 2);
    if (cnt[3]) k_tile_sort_blk<32><<<cnt[3], 256, 0, st>>>(T, ts, keys, point_list, cc, cl, 3);
    if (cnt[4]) k_tile_sort_big<<<cnt[4], SORT_BLOCK, 0, st>>>(T, ts, keys, point_list, cc, cl);
    return hipGetLastError();
}

}  // namespace lsr
