// lsr_api_common.h — what the three C-ABI driver files (lsr_api.hip,
// lsr_api_ops.hip, lsr_api_runtime.hip) share: the error macros, the
// process-wide options, the stage profiler and the debug guard.  Host-only.
#pragma once
#include <stdio.h>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>
#include "lsr_internal.h"

#define LSR_HIP(expr)                                                        \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) {                                              \
            fprintf(stderr, "[lsr] %s failed: %s (%s:%d)\n", #expr,          \
                    hipGetErrorString(_e), __FILE__, __LINE__);              \
            return LSR_EHIP;                                                 \
        }                                                                    \
    } while (0)

#define LSR_DEBUG_SYNC(s, st, stage)                                         \
    do {                                                                     \
        if ((s)->debug) {                                                    \
            hipError_t _e = hipStreamSynchronize(st);                        \
            if (_e == hipSuccess) _e = hipGetLastError();                    \
            if (_e != hipSuccess) {                                          \
                fprintf(stderr, "[lsr] stage %s failed: %s\n", stage,        \
                        hipGetErrorString(_e));                              \
                return LSR_EHIP;                                             \
            }                                                                \
        }                                                                    \
    } while (0)

// a step that returns an LSR_* code: anything but LSR_OK ends the caller with it
#define LSR_TRY(expr)                                     \
    do {                                                  \
        const int _rc = (expr);                           \
        if (_rc != LSR_OK) return _rc;                    \
    } while (0)

namespace lsr {

// ------------------------------------------------------------------ options
// Process-wide options (lsr_set_option), indexed by option id: the value and
// the range lsr_set_option accepts.  The table is in lsr_api_runtime.hip; the
// product path reads a value with one relaxed load.
struct Option {
    std::atomic<int64_t> value;
    int64_t lo, hi;
};
constexpr int kOptionEnd = LSR_OPT_DETERMINISTIC + 1;   // ids 1 .. kOptionEnd - 1
extern Option g_options[kOptionEnd];
inline int64_t option(int id) { return g_options[id].value.load(std::memory_order_relaxed); }

// ---------------------------------------------------------------- profiling
// Optional per-stage HIP-event timing (diagnostics for bench.py's roofline):
// when enabled, each stage is bracketed by two events recorded on the
// caller's stream; lsr_profile_query sums their elapsed times.
enum Stage { ST_PRE, ST_SCAN, ST_DUP, ST_SCAN_T, ST_SCATTER, ST_SORT, ST_RENDER, ST_GZERO, ST_RENDER_BWD,
             ST_PRE_BWD, ST_DET_BOUNDS, ST_DET_FINISH, ST_N };

// Process-wide (the autograd engine runs backward on its own thread, and the
// caller enables timing on its thread), thread-safe: the switch and mask are
// atomics read once per stage; the event pool is guarded by a mutex that is
// only taken while timing is on.  Off, the product path touches nothing.
struct Prof {
    std::atomic<bool> on{false};
    std::atomic<unsigned> mask{~0u};   // stages bracketed when on (lsr_profile_stages)
    std::mutex mu;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[ST_N];
    size_t used[ST_N] = {};
};
extern Prof g_prof;   // lsr_api_runtime.hip

struct StageScope {
    Stage s;
    hipStream_t st;
    bool on;
    size_t slot = 0;
    StageScope(Stage s_, hipStream_t st_) : s(s_), st(st_), on(g_prof.on.load(std::memory_order_relaxed) &&
                                                                 ((g_prof.mask.load(std::memory_order_relaxed) >> s_) & 1u))
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        auto& v = g_prof.ev[s];
        if (g_prof.used[s] == v.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            v.push_back({a, b});
        }
        slot = g_prof.used[s]++;
        (void)hipEventRecord(v[slot].first, st);
    }
    ~StageScope()
    {
        if (!on) return;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        (void)hipEventRecord(g_prof.ev[s][slot].second, st);
    }
};

// Debug-mode NaN/Inf guard: one streaming scan per array, a
// synchronous read of the flag, LSR_ENONFINITE naming the array.  Off unless
// settings.debug (which already synchronises after every stage).
struct Guard {
    const lsr_settings* s;
    lsr_alloc_fn alloc;
    void* ctx;
    hipStream_t st;
    uint32_t* flag = nullptr;
    Guard(const lsr_settings* s_, lsr_alloc_fn a_, void* c_, hipStream_t st_) : s(s_), alloc(a_), ctx(c_), st(st_) {}
    int check(const char* what, const float* p, size_t n)
    {
        if (!s->debug || !p || n == 0) return LSR_OK;
        return run([&] { return launch_nonfinite(p, n, flag, st); }, LSR_ENONFINITE,
                   "non-finite values (NaN/Inf) in", what);
    }
    // the binning lists a render is about to gather through (debug only)
    int check_lists(const char* what, const uint32_t* point_list, size_t M, int P, const uint32_t* tile_start, size_t T)
    {
        if (!s->debug || !tile_start || T == 0) return LSR_OK;
        return run([&] { return launch_check_lists(point_list, M, (uint32_t)P, tile_start, T, flag, st); }, LSR_ELISTS,
                   "corrupt binning lists before", what);
    }

private:
    // clear the flag word (allocated on first use), run the scan, read the flag back
    template <class Scan>
    int run(Scan&& scan, int code, const char* finding, const char* what)
    {
        if (!flag) {
            if (!alloc) return LSR_EINVAL;
            flag = (uint32_t*)alloc(ctx, 256, LSR_BUF_GUARD);
            if (!flag) return LSR_ENOMEM;
        }
        uint32_t h = 0;
        LSR_HIP(hipMemsetAsync(flag, 0, 4, st));
        LSR_HIP(scan());
        LSR_HIP(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st));
        LSR_HIP(hipStreamSynchronize(st));
        if (h) {
            fprintf(stderr, "[lsr] %s %s\n", finding, what);
            return code;
        }
        return LSR_OK;
    }
};

#define LSR_GUARD(g, what, p, n) LSR_TRY((g).check((what), (p), (n)))

}  // namespace lsr
