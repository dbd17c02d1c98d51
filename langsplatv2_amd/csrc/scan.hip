// scan.hip — device-wide scan of uint32 values with a 64-bit total: the tile
// starts of the global-atomic binning path (lsr_api.hip) and the destination
// offsets of the densify gather (densify.hip).
#include "lsr_internal.h"
#include "scan.h"

namespace lsr {

#define SCAN_ITEMS 16
#define SCAN_BLOCK 256
#define SCAN_TILE (SCAN_ITEMS * SCAN_BLOCK)

size_t scan_partials(size_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE + 1; }

// (kept as a function of its own: called directly, k_scan_apply compiles to a
// different schedule of the same instructions)
__device__ __forceinline__ uint64_t block_excl_scan_u64(uint64_t v, uint64_t* sh, uint64_t& total)
{
    return block_excl_scan_u64_n<SCAN_BLOCK>(v, sh, total);
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_reduce(const uint32_t* __restrict__ in, size_t n,
                                                            uint64_t* __restrict__ part)
{
    __shared__ uint64_t sh[SCAN_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++)
        if (base + k < n) s += in[base + k];
    uint64_t tot;
    block_excl_scan_u64(s, sh, tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_part(uint64_t* __restrict__ part, int nb)
{
    __shared__ uint64_t sh[SCAN_BLOCK / 64];
    uint64_t carry = 0;
    for (int base = 0; base < nb; base += SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        uint64_t v = i < nb ? part[i] : 0;
        uint64_t tot;
        uint64_t ex = block_excl_scan_u64(v, sh, tot);
        __syncthreads();
        if (i < nb) part[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) part[nb] = carry;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_apply(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                           size_t n, const uint64_t* __restrict__ part, int exclusive)
{
    __shared__ uint64_t sh[SCAN_BLOCK / 64];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        v[k] = (base + k < n) ? in[base + k] : 0u;
        s += v[k];
    }
    uint64_t tot;
    uint64_t run = block_excl_scan_u64(s, sh, tot) + part[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const uint64_t incl = run + v[k];
        if (base + k < n) out[base + k] = (uint32_t)(exclusive ? run : incl);
        run = incl;
    }
}

hipError_t launch_scan_u32(const uint32_t* in, uint32_t* out, uint64_t* part, size_t n, bool exclusive, hipStream_t st)
{
    const int nb = (int)((n + SCAN_TILE - 1) / SCAN_TILE);
    if (nb > 0) k_scan_reduce<<<nb, SCAN_BLOCK, 0, st>>>(in, n, part);
    k_scan_part<<<1, SCAN_BLOCK, 0, st>>>(part, nb);
    if (nb > 0) k_scan_apply<<<nb, SCAN_BLOCK, 0, st>>>(in, out, n, part, exclusive ? 1 : 0);
    return hipGetLastError();
}

}  // namespace lsr
