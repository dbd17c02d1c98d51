// lsr_api_runtime.hip — the C ABI's entry points that launch no kernel: error
// strings and versions, the process-wide options, the stage profiler's tables
// and the stream helpers.
#include <string.h>
#include "lsr_api_common.h"

namespace lsr {

Option g_options[kOptionEnd] = {
    {{0}, 0, -1},   // (no option 0)
    // LSR_OPT_BIN_MODE: the forward's tile binning; one mode is built (binning.hip:
    // scatter into tile buckets; tile_sort.hip: per-tile sort).  The depth-ordered mode of round 4
    // (order.hip) measured slower at every size (cfg5 scatter 4.55 vs 0.84 ms) and
    // was removed in round 5.
    {{LSR_BIN_AUTO}, LSR_BIN_AUTO, LSR_BIN_SORTED_TILES},
    // LSR_OPT_LISTS_MAX_MB: the backward's per-block candidate lists (128 B per
    // instance of capacity) are written only while they fit this budget; above it
    // the backward re-stages its candidates from the tile lists (same results,
    // measured 2.8 % slower at cfg3).  cfg3: 0.6 GB; cfg5 (M = 60 M): 7.7 GB -> off.
    {{2048}, 0, INT64_MAX},
    // LSR_OPT_SPLIT_PREPROCESS: the SH colour pass on a second stream, concurrent
    // with the binning (preprocess.hip k_preprocess_colour).
    {{1}, 0, 1},
    // LSR_OPT_DETERMINISTIC: the render backward's cross-block sums as 64-bit
    // fixed-point atomics (render_det.h det_shift), converted back by k_det_finish
    {{0}, 0, 1},
};

Prof g_prof;

}  // namespace lsr

using namespace lsr;

static const char* kStageNames[ST_N] = {"preprocess", "scan_tiles", "bin_count", "scan_tile_counts", "bin_scatter",
                                        "tile_sort", "render_fwd", "grad_zero", "render_bwd", "preprocess_bwd",
                                        "det_bounds", "det_finish"};

extern "C" {

const char* lsr_strerror(int code)
{
    switch (code) {
        case LSR_OK: return "success";
        case LSR_EINVAL: return "invalid argument (shapes, missing or conflicting inputs)";
        case LSR_EUNSUPPORTED: return "unsupported configuration (language dim / SH coefficients beyond the compiled sets)";
        case LSR_EHIP: return "HIP runtime or kernel launch failure";
        case LSR_ENOMEM: return "workspace allocation failed";
        case LSR_EOVERFLOW: return "num_rendered exceeds 32-bit instance indexing";
        case LSR_ENONFINITE: return "non-finite (NaN/Inf) values in an input or output (debug guard)";
        case LSR_ELISTS: return "corrupt binning lists: a Gaussian id out of range or tile ranges not monotone (debug check)";
        default: return "unknown error";
    }
}

int lsr_abi_version(void) { return LSR_ABI_VERSION; }

int lsr_max_lang_dim(void) { return 64; }

int lsr_set_option(int option, int64_t value)
{
    if (option < 1 || option >= kOptionEnd) return LSR_EINVAL;
    Option& o = g_options[option];
    if (value < o.lo || value > o.hi) return LSR_EINVAL;
    o.value.store(value, std::memory_order_relaxed);
    return LSR_OK;
}

int lsr_get_option(int option, int64_t* value)
{
    if (!value || option < 1 || option >= kOptionEnd) return LSR_EINVAL;
    *value = lsr::option(option);
    return LSR_OK;
}

int lsr_stream_create(void** stream)
{
    if (!stream) return LSR_EINVAL;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return LSR_EHIP;
    *stream = (void*)s;
    return LSR_OK;
}

int lsr_stream_destroy(void* stream)
{
    if (!stream) return LSR_EINVAL;
    return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? LSR_OK : LSR_EHIP;
}

void lsr_profile_enable(int on) { g_prof.on.store(on != 0); }

int lsr_profile_stages(const char* names)
{
    if (!names || !*names) { g_prof.mask.store(~0u); return LSR_OK; }
    unsigned m = 0;
    const char* p = names;
    while (*p) {
        const char* e = p;
        while (*e && *e != ',') e++;
        int hit = -1;
        for (int k = 0; k < ST_N; k++)
            if (strlen(kStageNames[k]) == (size_t)(e - p) && strncmp(kStageNames[k], p, (size_t)(e - p)) == 0) hit = k;
        if (hit < 0) return LSR_EINVAL;
        m |= 1u << hit;
        p = *e ? e + 1 : e;
    }
    g_prof.mask.store(m);
    return LSR_OK;
}

void lsr_profile_reset(void)
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (int k = 0; k < ST_N; k++) g_prof.used[k] = 0;
}

int lsr_profile_query(const char** names, double* ms, int64_t* calls, int max_stages)
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    int n = 0;
    for (int k = 0; k < ST_N && n < max_stages; k++, n++) {
        double tot = 0.0;
        for (size_t i = 0; i < g_prof.used[k]; i++) {
            float e = 0.f;
            if (hipEventSynchronize(g_prof.ev[k][i].second) != hipSuccess) return -LSR_EHIP;
            if (hipEventElapsedTime(&e, g_prof.ev[k][i].first, g_prof.ev[k][i].second) != hipSuccess) return -LSR_EHIP;
            tot += e;
        }
        if (names) names[n] = kStageNames[k];
        if (ms) ms[n] = tot;
        if (calls) calls[n] = (int64_t)g_prof.used[k];
    }
    return n;
}

}  // extern "C"
