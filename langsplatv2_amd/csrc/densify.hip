// densify.hip — GaussianModel.densify_and_prune and reset_opacity of the RGB
// phase (scene/gaussian_model.py:303-306, 352-504; train.py:246-258), behind
// lsr_densify_plan / lsr_densify_apply / lsr_reset_opacity.
//
// The reference makes three passes of boolean-index gathers and cats over the
// six parameters and their twelve Adam moments (clone-cat, split-cat + prune of
// the split parents, final prune).  The result is four stably compacted
// segments of the input rows:
//   0  originals neither split nor pruned         (parameters and moments copied)
//   1  clones that pass the prune test             (parameters copied, moments 0)
//   2  round-0 children that pass the prune test   (xyz, scaling computed, rest copied)
//   3  round-1 children, likewise
// so it is one gather.  Plan: k_classify writes three keep flags per row
// (segments 2 and 3 share theirs: both children of a parent have the same
// log-scales and opacity, hence the same prune verdict) into one (3, N) array,
// launch_scan_u32 turns it into destination offsets, k_fill writes for every
// destination row its source row and kind, k_counts the segment sizes the host
// reads back to size the outputs.  Apply: k_apply, one launch for all 18
// tensors, a grid-stride loop over chunks of 256 destination rows whose map
// entries sit in LDS; every lane writes one element (coalesced) and reads
// src[map[d] w + c] (contiguous runs of w floats).  No atomics: the output is a
// pure function of the inputs, bit for bit.
#include "lsr_internal.h"

namespace lsr {

namespace {

constexpr int DN_BLOCK = 256;
constexpr int DN_MAX_BLOCKS = 1024;    // classify grid (its per-block counts are summed by one block)
constexpr uint32_t DN_KIND_SHIFT = 30;   // map entry = source row | kind << 30 (N <= 2^28)
constexpr uint32_t DN_ROW_MASK = (1u << DN_KIND_SHIFT) - 1;
enum { DN_COPY = 0, DN_CLONE = 1, DN_CHILD0 = 2, DN_CHILD1 = 3 };

// the workspace: flags (3, N) u32 | offsets (3, N) u32 | map (2 N) u32 | scan partials u64 |
// per-block {clone, split} selections u32 | counts (6) i64
struct DensifyLayout {
    size_t flags, offsets, map, part, sel, counts, total;
};
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
DensifyLayout densify_layout(int64_t N)
{
    DensifyLayout L;
    const size_t n = (size_t)N;
    size_t o = 0;
    L.flags = o;   o = align256(o + 3 * n * 4);
    L.offsets = o; o = align256(o + 3 * n * 4);
    L.map = o;     o = align256(o + 2 * n * 4);
    L.part = o;    o = align256(o + scan_partials(3 * n) * 8);
    L.sel = o;     o = align256(o + (size_t)DN_MAX_BLOCKS * 2 * 4);
    L.counts = o;  o = align256(o + LSR_DENSIFY_COUNTS * 8);
    L.total = o;
    return L;
}

int stream_blocks(int64_t items_per_block_units, int cap)
{
    return (int)(items_per_block_units < cap ? (items_per_block_units > 0 ? items_per_block_units : 1) : cap);
}

int cu_count()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    return cus;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
// scaling_inverse_activation(get_scaling / (0.8 * 2)): the log-scale of a split child
__device__ __forceinline__ float child_scale(float s) { return logf(expf(s) / 1.6f); }

__global__ void __launch_bounds__(DN_BLOCK) k_classify(int64_t N, const float* __restrict__ accum,
                                                       const float* __restrict__ denom,
                                                       const float* __restrict__ scaling,
                                                       const float* __restrict__ opacity, DensifyArgs a,
                                                       uint32_t* __restrict__ flags, uint32_t* __restrict__ sel)
{
    uint32_t n_clone = 0, n_split = 0;
    const int64_t stride = (int64_t)gridDim.x * DN_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < N; i += stride) {
        float g = accum[i] / denom[i];
        if (g != g) g = 0.f;   // only NaN (0 / 0): x / 0 stays inf and is selected
        const float s0 = scaling[3 * i], s1 = scaling[3 * i + 1], s2 = scaling[3 * i + 2];
        const float ms = fmaxf(fmaxf(expf(s0), expf(s1)), expf(s2));
        // densify_and_clone tests the row norm of the (N, 1) gradient, densify_and_split the value
        const bool clone = fabsf(g) >= a.max_grad && ms <= a.dense_thresh;
        const bool split = g >= a.max_grad && ms > a.dense_thresh;
        const bool faint = sigmoidf(opacity[i]) < a.min_opacity;
        const bool gone = faint || (a.prune_big && ms > a.big_thresh);
        bool child = false;
        if (split) {
            const float cs = fmaxf(fmaxf(expf(child_scale(s0)), expf(child_scale(s1))), expf(child_scale(s2)));
            child = !(faint || (a.prune_big && cs > a.big_thresh));
        }
        flags[i] = (!split && !gone) ? 1u : 0u;
        flags[N + i] = (clone && !gone) ? 1u : 0u;
        flags[2 * N + i] = child ? 1u : 0u;
        n_clone += clone ? 1u : 0u;
        n_split += split ? 1u : 0u;
    }
    __shared__ uint32_t sh[2][DN_BLOCK / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n_clone += __shfl_down(n_clone, d, 64);
        n_split += __shfl_down(n_split, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = n_clone;
        sh[1][threadIdx.x >> 6] = n_split;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (int w = 0; w < DN_BLOCK / 64; w++) s += sh[threadIdx.x][w];
        sel[2 * blockIdx.x + threadIdx.x] = s;
    }
}

// counts = {segment 0..3 sizes, rows selected for cloning, rows selected for splitting}
__global__ void __launch_bounds__(64) k_counts(int64_t N, const uint32_t* __restrict__ offsets,
                                               const uint64_t* __restrict__ total, const uint32_t* __restrict__ sel,
                                               int blocks, int64_t* __restrict__ counts)
{
    if (threadIdx.x < 2) {
        int64_t s = 0;
        for (int b = 0; b < blocks; b++) s += sel[2 * b + threadIdx.x];
        counts[4 + threadIdx.x] = s;
    }
    if (threadIdx.x == 2) {
        const int64_t a = offsets[N], b = offsets[2 * N], t = (int64_t)*total;
        counts[0] = a;
        counts[1] = b - a;
        counts[2] = t - b;
        counts[3] = t - b;
    }
}

__global__ void __launch_bounds__(DN_BLOCK) k_fill(int64_t N, const uint32_t* __restrict__ flags,
                                                   const uint32_t* __restrict__ offsets,
                                                   const uint64_t* __restrict__ total, uint32_t* __restrict__ map)
{
    const uint32_t n_child = (uint32_t)*total - offsets[2 * N];
    const int64_t stride = (int64_t)gridDim.x * DN_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < N; i += stride) {
        const uint32_t row = (uint32_t)i;
        if (flags[i]) map[offsets[i]] = row | ((uint32_t)DN_COPY << DN_KIND_SHIFT);
        if (flags[N + i]) map[offsets[N + i]] = row | ((uint32_t)DN_CLONE << DN_KIND_SHIFT);
        if (flags[2 * N + i]) {
            const uint32_t d = offsets[2 * N + i];
            map[d] = row | ((uint32_t)DN_CHILD0 << DN_KIND_SHIFT);
            map[d + n_child] = row | ((uint32_t)DN_CHILD1 << DN_KIND_SHIFT);
        }
    }
}

// xyz of a split child, component c: build_rotation(q)[c, :] . (exp(scaling) * z) + xyz[c]
// (utils/general_utils.py:78-99; the quaternion is normalised here, as there)
__device__ __forceinline__ float child_xyz(const float* __restrict__ rot, const float* __restrict__ scaling,
                                           const float* __restrict__ xyz, const float* __restrict__ noise,
                                           int64_t src, int round, int c)
{
    const float q0 = rot[4 * src], q1 = rot[4 * src + 1], q2 = rot[4 * src + 2], q3 = rot[4 * src + 3];
    const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
    float R0, R1, R2;
    if (c == 0) {
        R0 = 1.f - 2.f * (y * y + z * z);
        R1 = 2.f * (x * y - r * z);
        R2 = 2.f * (x * z + r * y);
    } else if (c == 1) {
        R0 = 2.f * (x * y + r * z);
        R1 = 1.f - 2.f * (x * x + z * z);
        R2 = 2.f * (y * z - r * x);
    } else {
        R0 = 2.f * (x * z - r * y);
        R1 = 2.f * (y * z + r * x);
        R2 = 1.f - 2.f * (x * x + y * y);
    }
    const float* zn = noise + (src * 2 + round) * 3;
    const float v0 = expf(scaling[3 * src]) * zn[0];
    const float v1 = expf(scaling[3 * src + 1]) * zn[1];
    const float v2 = expf(scaling[3 * src + 2]) * zn[2];
    return ((R0 * v0 + R1 * v1) + R2 * v2) + xyz[3 * src + c];
}

enum { DN_PLAIN = 0, DN_XYZ = 1, DN_SCALING = 2, DN_MOMENT = 3 };

// one tensor's share of a chunk of `rows` destination rows starting at d0
template <int W>
__device__ __forceinline__ void gather_rows(const DensifyTable& t, int k, int w_rt, int role, int64_t d0, int rows,
                                            const uint32_t* __restrict__ smap)
{
    const int w = W > 0 ? W : w_rt;
    const float* __restrict__ src = t.src[k];
    float* __restrict__ dst = t.dst[k] + d0 * w;   // 64-bit element offset
    const int n = rows * w;
    for (int l = threadIdx.x; l < n; l += DN_BLOCK) {
        const int r = l / w, c = l - r * w;
        const uint32_t e = smap[r];
        const int kind = (int)(e >> DN_KIND_SHIFT);
        const int64_t s = (int64_t)(e & DN_ROW_MASK);
        float v;
        if (role == DN_MOMENT && kind != DN_COPY)
            v = 0.f;
        else if (role == DN_XYZ && kind >= DN_CHILD0)
            v = child_xyz(t.src[LSR_DENSIFY_ROTATION], t.src[LSR_DENSIFY_SCALING], src, t.noise, s,
                          kind - DN_CHILD0, c);
        else if (role == DN_SCALING && kind >= DN_CHILD0)
            v = child_scale(src[s * w + c]);
        else
            v = src[s * w + c];
        dst[l] = v;
    }
}

__global__ void __launch_bounds__(DN_BLOCK) k_apply(int64_t n_out, const uint32_t* __restrict__ map,
                                                  const int64_t* __restrict__ counts, DensifyTable t)
{
    __shared__ uint32_t smap[DN_BLOCK];
    // never past the rows the plan filled, whatever the caller sized its outputs to
    const int64_t planned = counts[0] + counts[1] + counts[2] + counts[3];
    n_out = n_out < planned ? n_out : planned;
    const int64_t chunks = (n_out + DN_BLOCK - 1) / DN_BLOCK;
    for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const int64_t d0 = ch * DN_BLOCK;
        const int rows = (int)(n_out - d0 < DN_BLOCK ? n_out - d0 : DN_BLOCK);
        __syncthreads();   // the previous chunk's readers are done
        if ((int)threadIdx.x < rows) smap[threadIdx.x] = map[d0 + threadIdx.x];
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < 3 * LSR_DENSIFY_GROUPS; k++) {
            if (!t.dst[k]) continue;
            const int grp = k % LSR_DENSIFY_GROUPS, w = t.width[grp];
            const int role = k >= LSR_DENSIFY_GROUPS ? DN_MOMENT
                             : grp == LSR_DENSIFY_XYZ ? DN_XYZ
                             : grp == LSR_DENSIFY_SCALING ? DN_SCALING : DN_PLAIN;
            switch (w) {   // compile-time widths: the row / column split without a division
            case 1: gather_rows<1>(t, k, w, role, d0, rows, smap); break;
            case 3: gather_rows<3>(t, k, w, role, d0, rows, smap); break;
            case 4: gather_rows<4>(t, k, w, role, d0, rows, smap); break;
            case 9: gather_rows<9>(t, k, w, role, d0, rows, smap); break;
            case 24: gather_rows<24>(t, k, w, role, d0, rows, smap); break;
            case 45: gather_rows<45>(t, k, w, role, d0, rows, smap); break;
            default: gather_rows<0>(t, k, w, role, d0, rows, smap); break;
            }
        }
    }
}

// opacity <- inverse_sigmoid(min(sigmoid(opacity), 0.01)); both moments <- 0
__global__ void __launch_bounds__(DN_BLOCK) k_reset_opacity(int64_t n, float* __restrict__ opacity,
                                                            float* __restrict__ m, float* __restrict__ v)
{
    const int64_t stride = (int64_t)gridDim.x * DN_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < n; i += stride) {
        const float p = fminf(sigmoidf(opacity[i]), 0.01f);
        opacity[i] = logf(p / (1.f - p));
        if (m) m[i] = 0.f;
        if (v) v[i] = 0.f;
    }
}

}  // namespace

size_t densify_workspace_bytes(int64_t N) { return densify_layout(N).total; }

hipError_t launch_densify_plan(int64_t N, const float* accum, const float* denom, const float* scaling,
                               const float* opacity, const DensifyArgs& a, void* ws, hipStream_t st)
{
    const DensifyLayout L = densify_layout(N);
    uint8_t* base = (uint8_t*)ws;
    uint32_t* flags = (uint32_t*)(base + L.flags);
    uint32_t* offsets = (uint32_t*)(base + L.offsets);
    uint32_t* map = (uint32_t*)(base + L.map);
    uint64_t* part = (uint64_t*)(base + L.part);
    uint32_t* sel = (uint32_t*)(base + L.sel);
    int64_t* counts = (int64_t*)(base + L.counts);
    const int blocks = stream_blocks((N + DN_BLOCK - 1) / DN_BLOCK, DN_MAX_BLOCKS);
    k_classify<<<blocks, DN_BLOCK, 0, st>>>(N, accum, denom, scaling, opacity, a, flags, sel);
    hipError_t e = launch_scan_u32(flags, offsets, part, (size_t)(3 * N), true, st);
    if (e != hipSuccess) return e;
    const uint64_t* total = part + (scan_partials((size_t)(3 * N)) - 1);
    k_counts<<<1, 64, 0, st>>>(N, offsets, total, sel, blocks, counts);
    k_fill<<<blocks, DN_BLOCK, 0, st>>>(N, flags, offsets, total, map);
    return hipGetLastError();
}

const int64_t* densify_counts(int64_t N, const void* ws)
{
    return (const int64_t*)((const uint8_t*)ws + densify_layout(N).counts);
}

hipError_t launch_densify_apply(int64_t N, int64_t n_out, const void* ws, const DensifyTable& t, hipStream_t st)
{
    if (n_out <= 0) return hipSuccess;
    const DensifyLayout L = densify_layout(N);
    const uint32_t* map = (const uint32_t*)((const uint8_t*)ws + L.map);
    const int64_t* counts = (const int64_t*)((const uint8_t*)ws + L.counts);
    const int blocks = stream_blocks((n_out + DN_BLOCK - 1) / DN_BLOCK, 8 * cu_count());
    k_apply<<<blocks, DN_BLOCK, 0, st>>>(n_out, map, counts, t);
    return hipGetLastError();
}

hipError_t launch_reset_opacity(int64_t n, float* opacity, float* m, float* v, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int blocks = stream_blocks((n + DN_BLOCK - 1) / DN_BLOCK, 8 * cu_count());
    k_reset_opacity<<<blocks, DN_BLOCK, 0, st>>>(n, opacity, m, v);
    return hipGetLastError();
}

}  // namespace lsr
