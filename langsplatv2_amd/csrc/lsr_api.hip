// lsr_api.hip — the render driver of the C ABI (include/lsr.h): lsr_forward and
// lsr_backward validate their arguments, request workspaces through the
// caller's allocator and enqueue the gfx950 kernels on the caller's stream.
// (The single-kernel entry points: lsr_api_ops.hip; options, profiling and
// stream helpers: lsr_api_runtime.hip.)
//
// Forward pipeline (one host sync, for num_rendered):
//   preprocess -> scan(tiles_touched) -> [read M] -> duplicate (tile ranks)
//   -> scan(tile counts) -> scatter into tile buckets -> per-tile depth sort
//   -> render (dense or quick)
// Backward: zero gradient rows -> render bwd (wave-reduced atomics)
//   -> preprocess bwd (chain rule, writes every requested output).
#include "lsr_api_common.h"

using namespace lsr;

namespace {

#ifndef LSR_SPLIT_MIN_P
#define LSR_SPLIT_MIN_P (1 << 19)
#endif
constexpr int kSplitPreMinP = LSR_SPLIT_MIN_P;

int guard_inputs(Guard& g, const lsr_settings* s, const lsr_inputs* in)
{
    const size_t P = (size_t)in->P;
    LSR_GUARD(g, "means3D", in->means3D, P * 3);
    LSR_GUARD(g, "opacities", in->opacities, P);
    LSR_GUARD(g, "shs", in->shs, P * (size_t)in->max_coeffs * 3);
    LSR_GUARD(g, "colors_precomp", in->colors_precomp, P * 3);
    LSR_GUARD(g, "scales", in->scales, P * 3);
    LSR_GUARD(g, "rotations", in->rotations, P * 4);
    LSR_GUARD(g, "cov3D_precomp", in->cov3D_precomp, P * 6);
    if (s->include_feature && !s->quick_render)
        LSR_GUARD(g, "language_feature_precomp", in->language_feature_precomp, P * (size_t)in->lang_dim);
    if (s->quick_render)
        LSR_GUARD(g, "language_feature_weights_quick", in->language_feature_weights_quick, P * (size_t)in->quick_k);
    return LSR_OK;
}

int dense_dim(const lsr_settings* s, const lsr_inputs* in)
{
    if (s->quick_render || !s->include_feature) return 0;
    return in->language_feature_precomp ? in->lang_dim : 0;
}

int quick_dim(const lsr_settings* s) { return s->quick_dim > 0 ? s->quick_dim : 192; }

int validate(const lsr_settings* s, const lsr_inputs* in)
{
    if (!s || !in) return LSR_EINVAL;
    if (s->image_height <= 0 || s->image_width <= 0 || in->P < 0) return LSR_EINVAL;
    if (!s->bg || !s->viewmatrix || !s->projmatrix || !s->campos) return LSR_EINVAL;
    if (s->quick_layout != LSR_LAYOUT_CHW && s->quick_layout != LSR_LAYOUT_HWC) return LSR_EINVAL;
    if (s->quick_layout == LSR_LAYOUT_HWC && !s->quick_render) return LSR_EINVAL;
    if (in->P > 0) {
        if (!in->means3D || !in->opacities) return LSR_EINVAL;
        if ((in->shs == nullptr) == (in->colors_precomp == nullptr)) return LSR_EINVAL;
        const bool sr = in->scales && in->rotations;
        if (sr == (in->cov3D_precomp != nullptr)) return LSR_EINVAL;
        if (in->shs && (in->max_coeffs <= 0 || s->sh_degree < 0 || s->sh_degree > 3 ||
                        (s->sh_degree + 1) * (s->sh_degree + 1) > in->max_coeffs))
            return LSR_EINVAL;
        if (in->shs && in->max_coeffs > 16) return LSR_EUNSUPPORTED;
    }
    if (s->quick_render) {
        if (in->P > 0 && (!in->language_feature_weights_quick || !in->language_feature_indices || in->quick_k <= 0))
            return LSR_EINVAL;
        if (in->quick_index_dtype < LSR_INDEX_F32 || in->quick_index_dtype > LSR_INDEX_PACKED) return LSR_EINVAL;
        // the 12-code LDS-DMA kernel stages 16-B aligned rows
        const bool dma_rows = in->quick_k == 12 &&
                              (in->P == 0 || (((uintptr_t)in->language_feature_weights_quick % 16) == 0 &&
                                              ((uintptr_t)in->language_feature_indices % 16) == 0));
        // packed rows: that kernel's staging format
        if (in->quick_index_dtype == LSR_INDEX_PACKED && (!dma_rows || quick_dim(s) > 192)) return LSR_EUNSUPPORTED;
        if ((size_t)quick_dim(s) * 256 + 64 * (32 + 12 + 8 * (size_t)in->quick_k) > 65536) return LSR_EUNSUPPORTED;
        // the pixel-major map is written by that kernel at 192 channels only
        if (s->quick_layout == LSR_LAYOUT_HWC && (!dma_rows || quick_dim(s) != 192)) return LSR_EUNSUPPORTED;
    } else if (s->include_feature) {
        if (in->P > 0 && (!in->language_feature_precomp || in->lang_dim <= 0)) return LSR_EINVAL;
        if (lang_set_for(in->lang_dim) < 0) return LSR_EUNSUPPORTED;
    }
    return LSR_OK;
}

Cam make_cam(const lsr_settings* s)
{
    Cam c;
    c.W = s->image_width;
    c.H = s->image_height;
    c.gx = (c.W + LSR_TILE - 1) / LSR_TILE;
    c.gy = (c.H + LSR_TILE - 1) / LSR_TILE;
    c.tanfovx = s->tanfovx;
    c.tanfovy = s->tanfovy;
    c.fx = (float)c.W / (2.0f * s->tanfovx);
    c.fy = (float)c.H / (2.0f * s->tanfovy);
    c.scale_modifier = s->scale_modifier;
    c.view = s->viewmatrix;
    c.proj = s->projmatrix;
    c.campos = s->campos;
    c.bg = s->bg;
    c.sh_degree = s->sh_degree;
    return c;
}

RenderArgs make_render_args(const lsr_settings* s, const lsr_inputs* in, const Cam& c, const uint8_t* geom,
                            const uint8_t* bin, const uint8_t* img, int64_t M)
{
    RenderArgs a;
    const GeomLayout GL = geom_layout((size_t)in->P);
    const int T = c.gx * c.gy;
    const ImageLayout IL = image_layout((size_t)c.W * c.H, (size_t)T);
    const BinLayout BL = bin_layout((size_t)M);
    a.cam = c;
    a.P = in->P;
    a.splatA = (const float4*)(geom + GL.splatA);
    a.splatB = (const float4*)(geom + GL.splatB);
    a.rgb = in->colors_precomp ? in->colors_precomp : (const float*)(geom + GL.rgb);
    a.D = dense_dim(s, in);
    a.lang = a.D ? in->language_feature_precomp : nullptr;
    a.qw = s->quick_render ? in->language_feature_weights_quick : nullptr;
    a.qi = s->quick_render ? in->language_feature_indices : nullptr;
    a.qidx_dtype = in->quick_index_dtype;
    a.K = s->quick_render ? in->quick_k : 0;
    a.Dq = s->quick_render ? quick_dim(s) : 0;
    a.quick_hwc = s->quick_render && s->quick_layout == LSR_LAYOUT_HWC;
    a.point_list = (const uint32_t*)(bin + BL.point_list);
    a.tile_start = (const uint32_t*)(img + IL.tile_start);
    a.final_T = (float*)(img + IL.final_T);
    a.n_contrib = (uint32_t*)(img + IL.n_contrib);
    a.out_color = nullptr;
    a.out_lang = nullptr;
    return a;
}

// ------------------------------------------- split preprocess: colour stream
// One non-blocking stream and two events per host thread and device (created
// on first use, destroyed when the thread exits), on the device of the
// caller's stream (not the thread's current device: a caller may pass another
// device's stream).  The SH colour pass runs there behind the geometry pass
// while the caller's stream bins.  When no colour stream can be had (device
// index >= 16, creation failure) the forward runs the fused preprocess, which
// gives identical results.
struct ColourStream {
    hipStream_t stream = nullptr;
    hipEvent_t geom_done = nullptr, colour_done = nullptr;
    void release()
    {
        if (colour_done) (void)hipEventDestroy(colour_done);
        if (geom_done) (void)hipEventDestroy(geom_done);
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        geom_done = colour_done = nullptr;
    }
    ~ColourStream() { release(); }
};

ColourStream* colour_stream(hipStream_t st)
{
    thread_local ColourStream tab[16];
    hipDevice_t sdev = 0;
    int cur = 0;
    if (hipStreamGetDevice(st, &sdev) != hipSuccess || hipGetDevice(&cur) != hipSuccess) return nullptr;
    const int dev = (int)sdev;
    if (dev < 0 || dev >= 16) return nullptr;
    ColourStream& cs = tab[dev];
    if (!cs.stream) {
        // streams and events belong to the device current at their creation
        if (dev != cur && hipSetDevice(dev) != hipSuccess) return nullptr;
        const bool ok = hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking) == hipSuccess &&
                        hipEventCreateWithFlags(&cs.geom_done, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&cs.colour_done, hipEventDisableTiming) == hipSuccess;
        if (dev != cur) (void)hipSetDevice(cur);
        if (!ok) {
            cs.release();
            return nullptr;
        }
    }
    return &cs;
}

// Makes the caller's stream wait for the colour pass exactly once: before the
// render, or on any early return (the pass writes into the caller's geometry
// buffer, which must not be released while it runs).
struct ColourJoin {
    ColourStream* cs;
    hipStream_t st;
    bool done = false;
    hipError_t wait()
    {
        if (!cs || done) return hipSuccess;
        done = true;
        return hipStreamWaitEvent(st, cs->colour_done, 0);
    }
    ~ColourJoin() { (void)wait(); }
};

// ------------------------------------------------- host-visible scan total
// One coherent pinned line per host thread: word 0 receives (seq << 32 | M)
// from k_bin_count (k_publish_total on the global-atomic path), the u32 words
// 2 .. 1 + SORT_NCLS (inside u64 words 1..3) the tile-sort class counts and
// word LSR_CLS_SLOT (seq << 32 | M) once those are out (k_bin_table); the host
// spins until a word's sequence matches.
struct HostSlot {
    uint64_t* word = nullptr;   // host view
    uint64_t* dev = nullptr;    // device view of the same word
    uint32_t seq = 0;
    uint64_t last_m = 0;        // previous forward's M (binning size guess)
    ~HostSlot() { if (word) (void)hipHostFree(word); }
};

HostSlot& host_slot()
{
    thread_local HostSlot hs;
    if (!hs.word) {
        void* p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
            return hs;
        void* d = nullptr;
        if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipHostFree(p); return hs; }
        hs.word = (uint64_t*)p;
        hs.dev = (uint64_t*)d;
        *(volatile uint64_t*)hs.word = 0;
    }
    return hs;
}

// Spin on the published word; every 4096 polls ask the runtime whether the
// stream has drained (which also covers a stream the runtime has not
// submitted yet, and reports a faulted stream instead of spinning forever).
int wait_published(HostSlot& hs, uint32_t seq, hipStream_t st, uint64_t* M, int slot = 0)
{
    auto published = [&] {
        const uint64_t v = __atomic_load_n(hs.word + slot, __ATOMIC_ACQUIRE);
        if ((uint32_t)(v >> 32) != seq) return false;
        *M = v & 0xffffffffull;
        return true;
    };
    for (uint64_t it = 1;; it++) {
        if (published()) return LSR_OK;
        if ((it & 4095) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) {
                if (published()) return LSR_OK;
                fprintf(stderr, "[lsr] scan total was not published (stream drained)\n");
                return LSR_EHIP;
            }
            if (q != hipErrorNotReady) {
                fprintf(stderr, "[lsr] stream failed while waiting for the scan total: %s\n", hipGetErrorString(q));
                return LSR_EHIP;
            }
        }
        __builtin_ia32_pause();
    }
}

// ------------------------------------------------------- the backward's plan
// The dense backward's shape, decided here alone -- by the forward, which
// prepares the accumulators (lsr_fwd_out.grad_ws / grad_ws_lang), and by the
// backward, which runs it: gradient rows (P x VP, unless only dL/dlang is
// requested) and, where the render backward adds dL/dlang straight into an
// (P, D) array (language-only, or D = 16 / 32 with 16-B aligned rows, which
// the kernel gathers as float4 lines), that array -- a separate allocation,
// so the gradient the caller keeps holds no gradient rows alive.  kind encodes
// the configuration, so a backward uses a forward's accumulators only when it
// needs exactly these.
struct BwdPlan {
    int kind = 0;          // 0: nothing for a forward to prepare
    int VP = 0;            // gradient row width (0: language-only, no rows)
    size_t rows_bytes = 0, lang_bytes = 0;
    // lang_only: only dL/dlanguage requested (feature-mode training with frozen
    // geometry and no means2D gradient): the language-only render backward
    // writes the output directly; no gradient rows, no preprocess backward.
    // lang_direct: the full render backward adds the language gradients
    // straight into the output; the rows keep geometry + colour (one 64-B
    // line) and preprocess_bwd no longer copies language.
    bool lang_only = false, lang_direct = false;
};
BwdPlan plan_backward(int P, int Dd, bool geom, bool lang, const float* lang_rows)
{
    BwdPlan w;
    lang = lang && Dd > 0;
    w.lang_only = lang && !geom;
    w.lang_direct = lang && geom && bwd_lang_direct(Dd) && (uintptr_t)lang_rows % 16 == 0;
    if (!w.lang_only) w.VP = w.lang_direct ? 16 : grad_row_width(Dd);
    w.rows_bytes = (size_t)P * w.VP * 4;
    if (w.lang_only || w.lang_direct) w.lang_bytes = (size_t)P * Dd * 4;
    // (neither requested: the backward still runs on rows of this width and writes no output)
    if (P > 0 && (geom || lang)) w.kind = (geom ? 1 : 0) | (lang ? 2 : 0) | (w.lang_direct ? 4 : 0) | (w.VP << 8);
    return w;
}

// The backward's per-block candidate lists (RenderArgs::listA/B/lcount): A and
// B arrays of 4 M entries (block b = 4 tile + sub owns [4 tile_start + sub n_tile,
// + n_tile)), then the 4 T per-block counts.  The forward that writes them also
// writes the backward's block order (RenderArgs::border, ImageLayout::border).
size_t block_lists_bytes(size_t M, size_t T)
{
    if (M == 0 || T == 0) return 0;
    return 2 * align256(4 * M * 16) + align256(4 * T * 4);
}
void set_block_lists(RenderArgs& ra, void* lb, size_t M)
{
    uint8_t* p = (uint8_t*)lb;
    ra.listA = (float4*)p;
    ra.listB = (float4*)(p + align256(4 * M * 16));
    ra.lcount = (uint32_t*)(p + 2 * align256(4 * M * 16));
}
// the backward's view of the lists, with the block order the same forward wrote
void set_block_lists_bwd(RenderArgs& ra, const void* lb, const void* img, size_t M)
{
    set_block_lists(ra, (void*)lb, M);
    const size_t T = (size_t)ra.cam.gx * ra.cam.gy;
    if (bwd_order_on((int)T)) ra.border = (const uint4*)((const uint8_t*)img + image_layout((size_t)ra.cam.W * ra.cam.H, T).border);
}

// ------------------------------------------------------------ forward stages
// The binning's shape: privatised (per-block tile histograms in a B x T table
// at the tail of the image workspace) where the image fits the LDS band, else
// the global-atomic path.
struct BinShape {
    bool priv;
    int chunk = 0, B = 0;
    size_t table_bytes = 0;
    BinShape(const Cam& c, int P) : priv(P > 0 && bin_privatised_ok(c))
    {
        if (!priv) return;
        B = bin_blocks(P, c, chunk);
        table_bytes = align256((size_t)B * table_stride(c.gx * c.gy) * 4);
    }
};

// Bin: count the (Gaussian, tile) instances, read their number M on the host
// (the forward's one sync), scatter the instances into their tiles' buckets
// and sort each bucket by depth.  Leaves M in out->num_rendered and the
// binning workspace in out->binning.
int bin_tiles(const lsr_settings* s, const Cam& c, int P, const BinShape& bs, uint8_t* geom, uint8_t* img,
              lsr_fwd_out* out, lsr_alloc_fn alloc, void* ctx, hipStream_t st)
{
    const int T = c.gx * c.gy;
    const GeomLayout GL = geom_layout((size_t)P);
    const ImageLayout IL = image_layout((size_t)c.W * c.H, (size_t)T);
    const BinWs ws{bs.chunk, bs.B, (uint32_t*)(img + IL.total), (uint32_t*)(img + IL.tile_cnt),
                   (uint32_t*)(img + IL.tile_start), (uint64_t*)(img + IL.tile_part), (uint32_t*)(img + IL.cls_cnt),
                   (uint32_t*)(img + IL.cls_list)};
    const size_t tnb = scan_partials((size_t)T) - 1;

    HostSlot& hs = host_slot();
    if (!hs.word) return LSR_EHIP;
    const uint32_t seq = ++hs.seq;
    const HostWord hw{hs.dev, seq};
    if (bs.priv) {
        // per-block tile histograms -> column scan -> tile starts; M = total
        {
            StageScope sc(ST_DUP, st);
            LSR_HIP(launch_bin_count(c, P, geom, out->radii, ws, hw, st));
        }
        {
            StageScope sc(ST_SCAN_T, st);
            LSR_HIP(launch_tile_start_apply(T, ws, st));
        }
    } else {
        uint64_t* gpart = (uint64_t*)(geom + GL.scan_part);
        const size_t gnb = scan_partials((size_t)P) - 1;
        StageScope sc(ST_SCAN, st);
        LSR_HIP(launch_scan_u32((const uint32_t*)(geom + GL.tiles), (uint32_t*)(geom + GL.offsets), gpart,
                                (size_t)P, false, st));
        LSR_HIP(launch_publish_total(gpart + gnb, hw, st));
    }
    // speculative binning workspace sized from the previous call's M, taken
    // while the GPU is still counting, so the host usually has nothing but
    // launches to do once M is known
    uint8_t* bin = nullptr;
    size_t bin_cap = 0;
    if (hs.last_m > 0) {
        const size_t guess = (size_t)(hs.last_m + hs.last_m / 4 + 4096);
        bin_cap = bin_layout(guess).total;
        bin = (uint8_t*)alloc(ctx, bin_cap, LSR_BUF_BINNING);
        if (!bin) return LSR_ENOMEM;
    }
    uint64_t M = 0;
    LSR_TRY(wait_published(hs, seq, st, &M));
    LSR_DEBUG_SYNC(s, st, "count");
    if (M >= 0xffffffffull) return LSR_EOVERFLOW;
    out->num_rendered = (int64_t)M;
    hs.last_m = M;

    // binning workspace + scatter into tile buckets
    const BinLayout BL = bin_layout((size_t)M);
    if (!bin || BL.total > bin_cap) {
        bin_cap = BL.total > 0 ? BL.total : 256;
        bin = (uint8_t*)alloc(ctx, bin_cap, LSR_BUF_BINNING);
        if (!bin) return LSR_ENOMEM;
    }
    out->binning = bin;
    out->binning_bytes = bin_cap;
    if (bs.priv) {
        StageScope sc(ST_SCATTER, st);
        LSR_HIP(launch_bin_scatter(c, P, geom, out->radii, ws, (uint64_t*)(bin + BL.keys), st));
    } else {
        {
            StageScope sc(ST_DUP, st);
            LSR_HIP(hipMemsetAsync(ws.tile_cnt, 0, (size_t)T * 4, st));
            LSR_HIP(launch_duplicate(c, P, geom, out->radii, ws.tile_cnt, (uint32_t*)(bin + BL.rank), st));
        }
        {
            StageScope sc(ST_SCAN_T, st);
            LSR_HIP(launch_scan_u32(ws.tile_cnt, ws.tile_start, ws.tpart, (size_t)T, true, st));
            LSR_HIP(hipMemcpyAsync(ws.tile_start + T, ws.tpart + tnb, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        }
        StageScope sc(ST_SCATTER, st);
        LSR_HIP(launch_scatter(c, P, geom, out->radii, ws.tile_start, (const uint32_t*)(bin + BL.rank),
                               (uint64_t*)(bin + BL.keys), st));
    }
    LSR_DEBUG_SYNC(s, st, "scatter");
    // the privatised path's tile-sort class counts: published by the column
    // scan (k_bin_table) with its own M, after the count published M -- the
    // scatter above was launched in between
    uint32_t host_cls[SORT_NCLS];
    if (bs.priv) {
        uint64_t M2 = 0;
        LSR_TRY(wait_published(hs, seq, st, &M2, LSR_CLS_SLOT));
        if (M2 != M) {
            fprintf(stderr, "[lsr] tile count and column scan disagree on M (%llu vs %llu)\n",
                    (unsigned long long)M, (unsigned long long)M2);
            return LSR_EHIP;
        }
        for (int k = 0; k < SORT_NCLS; k++) host_cls[k] = ((volatile uint32_t*)(hs.word + 1))[k];
    }
    {
        StageScope sc(ST_SORT, st);
        LSR_HIP(launch_tile_sort(T, ws, (uint64_t*)(bin + BL.keys), (uint32_t*)(bin + BL.point_list),
                                 bs.priv ? host_cls : nullptr, st));
    }
    LSR_DEBUG_SYNC(s, st, "tile_sort");
    return LSR_OK;
}

// A pending dense backward (out->grad_ws_request): its accumulators, which
// the render zeroes alongside its own work (ra.zero / zero2), and, within the
// LSR_OPT_LISTS_MAX_MB budget, the per-block candidate lists the render writes.
int prepare_backward(const lsr_settings* s, const lsr_inputs* in, int Dd, lsr_fwd_out* out, RenderArgs& ra,
                     lsr_alloc_fn alloc, void* ctx)
{
    out->grad_ws = out->grad_ws_lang = out->lists = nullptr;
    out->grad_ws_bytes = out->lists_bytes = 0;
    out->grad_ws_kind = 0;
    if (!out->grad_ws_request || s->quick_render) return LSR_OK;
    const BwdPlan w = plan_backward(in->P, Dd, (out->grad_ws_request & LSR_GWS_GEOM) != 0,
                                    (out->grad_ws_request & LSR_GWS_LANG) != 0, in->language_feature_precomp);
    if (!w.kind) return LSR_OK;
    // an accumulator in whole 256-B lines, for the render to zero
    auto zeroed = [&](size_t bytes, int tag, float4*& zero, size_t& n16) {
        zero = (float4*)alloc(ctx, align256(bytes), tag);
        n16 = align256(bytes) / 16;
        return (void*)zero;
    };
    if (w.rows_bytes) {
        if (!(out->grad_ws = zeroed(w.rows_bytes, LSR_BUF_GRAD, ra.zero, ra.zero_n16))) return LSR_ENOMEM;
        out->grad_ws_bytes = w.rows_bytes;
    }
    if (w.lang_bytes && !(out->grad_ws_lang = zeroed(w.lang_bytes, LSR_BUF_GRAD_LANG, ra.zero2, ra.zero2_n16)))
        return LSR_ENOMEM;
    out->grad_ws_kind = w.kind;
    // the backward's per-block candidate lists (render_fwd.hip ZERO / render_bwd.hip LST): the render
    // writes each 8x8 block's staged candidates; capacity 4 entries per instance
    const size_t M = (size_t)out->num_rendered;
    const size_t L = block_lists_bytes(M, (size_t)ra.cam.gx * ra.cam.gy);
    if (L && L <= ((size_t)option(LSR_OPT_LISTS_MAX_MB) << 20)) {
        void* lb = alloc(ctx, L, LSR_BUF_LISTS);
        if (!lb) return LSR_ENOMEM;
        out->lists = lb;
        out->lists_bytes = L;
        set_block_lists(ra, lb, M);
    }
    return LSR_OK;
}

// ----------------------------------------------------------- backward pieces
int guard_bwd_outputs(Guard& g, const lsr_inputs* in, const lsr_bwd_out* o, int D)
{
    const size_t P = (size_t)in->P;
    LSR_GUARD(g, "dL_dmeans2D", o->dL_dmeans2D, P * 3);
    LSR_GUARD(g, "dL_dcolors", o->dL_dcolors, P * 3);
    LSR_GUARD(g, "dL_dlang", o->dL_dlang, P * (size_t)D);
    LSR_GUARD(g, "dL_dopacity", o->dL_dopacity, P);
    LSR_GUARD(g, "dL_dmeans3D", o->dL_dmeans3D, P * 3);
    LSR_GUARD(g, "dL_dcov3D", o->dL_dcov3D, P * 6);
    LSR_GUARD(g, "dL_dsh", o->dL_dsh, P * (size_t)in->max_coeffs * 3);
    LSR_GUARD(g, "dL_dscales", o->dL_dscales, P * 3);
    LSR_GUARD(g, "dL_drotations", o->dL_drotations, P * 4);
    LSR_GUARD(g, "dL_dlang_weights", o->dL_dlang_weights, P * (size_t)in->quick_k);
    LSR_GUARD(g, "dL_drgb_sh", o->dL_drgb_sh, P * 3);
    return LSR_OK;
}

bool geometry_requested(const lsr_bwd_out* o)
{
    return o->dL_dmeans2D || o->dL_dcolors || o->dL_dopacity || o->dL_dmeans3D || o->dL_dcov3D || o->dL_dsh ||
           o->dL_dscales || o->dL_drotations || o->dL_drgb_sh;
}

int record_lang_ready(const lsr_bwd_out* out, hipStream_t st)
{
    if (out->lang_ready_event) LSR_HIP(hipEventRecord((hipEvent_t)out->lang_ready_event, st));
    return LSR_OK;
}

// The render backward's arguments over a saved forward: its workspaces, the
// block lists and block order where that forward wrote them (the sparse
// kernel has no list form and ignores them) and the upstream gradients of the
// D language channels it differentiates.  The caller adds the accumulators of
// its path: grad_acc + VP, lang_acc or qw_acc.
RenderBwdArgs make_render_bwd_args(const lsr_settings* s, const lsr_inputs* in, const lsr_bwd_in* b, int D)
{
    RenderBwdArgs rb;
    rb.f = make_render_args(s, in, make_cam(s), (const uint8_t*)b->geom, (const uint8_t*)b->binning,
                            (const uint8_t*)b->image, b->num_rendered);
    if (b->lists) set_block_lists_bwd(rb.f, b->lists, b->image, (size_t)b->num_rendered);
    rb.f.D = D;
    rb.dout_color = b->dL_dout_color;
    rb.dout_lang = D ? b->dL_dout_lang : nullptr;
    rb.grad_acc = nullptr;
    rb.VP = 0;
    return rb;
}

// LSR_OPT_DETERMINISTIC: the bounds word ({max |dL/dout|, max |feature|,
// flags}) and the zeroed 64-bit fixed-point twins of the accumulators the
// render backward adds into (rb.grad_acc's (P, VP) rows, and with lang_direct
// the (P, D) language rows); rb.radii = the forward's radii.
int det_prepare(RenderBwdArgs& rb, const int32_t* radii, bool lang_direct, lsr_alloc_fn alloc, void* ctx,
                hipStream_t st)
{
    rb.radii = radii;
    const size_t P = (size_t)rb.f.P;
    const size_t rows = align256(P * (size_t)rb.VP * 8);
    const size_t lang = lang_direct ? align256(P * (size_t)rb.f.D * 8) : 0;
    const size_t hdr = LSR_DET_HDR + align256(P * 4);   // + the shift table
    uint8_t* ws = (uint8_t*)alloc(ctx, hdr + rows + lang, LSR_BUF_DET);
    if (!ws) return LSR_ENOMEM;
    rb.det_bounds = (float*)ws;
    rb.det_sh = (uint32_t*)(ws + LSR_DET_HDR);
    rb.det_rows = (long long*)(ws + hdr);
    rb.det_lang = lang_direct ? (long long*)(ws + hdr + rows) : nullptr;
    {
        // the header and the shift table are written whole by launch_det_bounds
        StageScope sc(ST_DET_BOUNDS, st);
        LSR_HIP(launch_det_bounds(rb, rb.det_bounds, st));
    }
    // after the bounds pass: its reads would otherwise pay for writing the
    // cleared lines back from the last-level cache (bounds 0.094 -> 0.079 ms)
    StageScope sc(ST_GZERO, st);
    LSR_HIP(hipMemsetAsync(ws + hdr, 0, rows + lang, st));
    return LSR_OK;
}

// The dense-input backward (lsr_backward's body past validation; also the
// geometry path of the quick input, with that call's guard).
int backward_dense(const lsr_settings* s, const lsr_inputs* in, const lsr_bwd_in* b, lsr_bwd_out* out,
                   lsr_alloc_fn alloc, void* ctx, hipStream_t st, Guard& guard)
{
    const int Dd = dense_dim(s, in);
    if (Dd > 0 && !b->dL_dout_lang) return LSR_EINVAL;
    const BwdPlan W = plan_backward(in->P, Dd, geometry_requested(out), out->dL_dlang != nullptr,
                                    in->language_feature_precomp);
    // the forward's zeroed accumulators, when they are exactly what this call needs
    const bool ws_kind = W.kind != 0 && b->grad_ws_kind == W.kind;
    const bool ws_ok = ws_kind && W.rows_bytes > 0 && b->grad_ws && b->grad_ws_bytes >= W.rows_bytes;
    const bool ws_lang = ws_kind && W.lang_bytes > 0 && b->grad_ws_lang && out->dL_dlang == (float*)b->grad_ws_lang;
    const bool det = option(LSR_OPT_DETERMINISTIC) != 0;
    RenderBwdArgs rb = make_render_bwd_args(s, in, b, Dd);
    rb.VP = W.lang_only ? Dd : W.VP;   // (language-only: the accumulator is the (P, D) output itself)
    if (W.lang_only) {
        rb.grad_acc = out->dL_dlang;
        if (det) {
            LSR_TRY(det_prepare(rb, b->radii, false, alloc, ctx, st));
        } else if (!ws_lang) {
            StageScope sc(ST_GZERO, st);
            LSR_HIP(hipMemsetAsync(out->dL_dlang, 0, W.lang_bytes, st));
        }
        { StageScope sc(ST_RENDER_BWD, st); LSR_HIP(launch_render_bwd_lang(rb, st)); }
        if (det) { StageScope sc(ST_DET_FINISH, st); LSR_HIP(launch_det_finish(rb, true, nullptr, out->dL_dlang, st)); }
        LSR_DEBUG_SYNC(s, st, "render_bwd_lang");
        LSR_TRY(record_lang_ready(out, st));
        return guard_bwd_outputs(guard, in, out, Dd);
    }
    float* gacc = ws_ok ? (float*)b->grad_ws : (float*)alloc(ctx, W.rows_bytes, LSR_BUF_GRAD);
    if (!gacc) return LSR_ENOMEM;
    // (deterministic: k_det_finish writes every element of gacc and dL/dlang)
    if (!det && (!ws_ok || (W.lang_direct && !ws_lang))) {
        StageScope sc(ST_GZERO, st);
        if (!ws_ok) LSR_HIP(hipMemsetAsync(gacc, 0, W.rows_bytes, st));
        if (W.lang_direct && !ws_lang) LSR_HIP(hipMemsetAsync(out->dL_dlang, 0, W.lang_bytes, st));
    }
    rb.grad_acc = gacc;
    rb.lang_acc = W.lang_direct ? out->dL_dlang : nullptr;
    if (det) LSR_TRY(det_prepare(rb, b->radii, W.lang_direct, alloc, ctx, st));
    { StageScope sc(ST_RENDER_BWD, st); LSR_HIP(launch_render_bwd(rb, st)); }
    if (det) {
        StageScope sc(ST_DET_FINISH, st);
        LSR_HIP(launch_det_finish(rb, false, gacc, rb.lang_acc, st));
    }
    LSR_DEBUG_SYNC(s, st, "render_bwd");
    // the language gradient is final here unless preprocess_bwd copies it out
    const bool lang_final = W.lang_direct || !out->dL_dlang;
    if (lang_final) LSR_TRY(record_lang_ready(out, st));

    lsr_inputs in2 = *in;
    in2.lang_dim = Dd;
    lsr_bwd_out o2 = *out;
    if (!Dd || W.lang_direct) o2.dL_dlang = nullptr;
    {
        StageScope sc(ST_PRE_BWD, st);
        LSR_HIP(launch_preprocess_bwd(rb.f.cam, in2, (const uint8_t*)b->geom, b->radii, gacc, W.VP, o2, st));
    }
    LSR_DEBUG_SYNC(s, st, "preprocess_bwd");
    if (!lang_final) LSR_TRY(record_lang_ready(out, st));
    return guard_bwd_outputs(guard, in, out, Dd);
}

int zero_weight_grads(const lsr_inputs* in, float* dw, hipStream_t st)
{
    LSR_HIP(hipMemsetAsync(dw, 0, (size_t)in->P * in->quick_k * 4, st));
    return LSR_OK;
}

// Quick (sparse) language input: weights (P,K) + codes (P,K) rendered into
// Dq channels.  dL/dweights[j][m] = sum_p aT_j(p) dL/dout_lang[idx[j][m]][p].
//  - weights alone requested (feature-mode training, geometry frozen): the
//    language-only render backward gathers the channel gradients at the codes
//    (no dense (P,Dq) rows anywhere);
//  - geometry requested too: the quick channels take part in dL/dalpha when
//    their upstream gradient is given, so the sparse rows are expanded to
//    dense (P,Dq) rows and the dense backward runs (Dq <= 64), dL/dweights
//    gathered from its dL/dlang; without an upstream language gradient the
//    backward is the RGB-only one.
int backward_quick(const lsr_settings* s, const lsr_inputs* in, const lsr_bwd_in* b, lsr_bwd_out* out,
                   lsr_alloc_fn alloc, void* ctx, hipStream_t st, Guard& guard)
{
    const int P = in->P;
    const int Dq = quick_dim(s);
    float* dw = out->dL_dlang_weights;
    const bool geom = geometry_requested(out);
    if (!dw && !geom) return record_lang_ready(out, st);
    if (dw && !geom && !b->dL_dout_lang) {
        // the weights requested but the language output received no gradient
        // (autograd passes none when the loss ignores it): dL/dweights = 0
        LSR_TRY(zero_weight_grads(in, dw, st));
        return record_lang_ready(out, st);
    }
    // (deterministic mode: the expansion path below, whose dense language-only
    // backward sums in fixed point; the sparse gather adds floats in any order)
    if (dw && !geom && !option(LSR_OPT_DETERMINISTIC)) {
        if (lang_set_for(Dq) < 0) return LSR_EUNSUPPORTED;
        RenderBwdArgs rb = make_render_bwd_args(s, in, b, Dq);
        rb.VP = Dq;
        rb.qw_acc = dw;
        { StageScope sc(ST_GZERO, st); LSR_TRY(zero_weight_grads(in, dw, st)); }
        { StageScope sc(ST_RENDER_BWD, st); LSR_HIP(launch_render_bwd_lang_sparse(rb, st)); }
        LSR_DEBUG_SYNC(s, st, "render_bwd_lang_sparse");
        LSR_TRY(record_lang_ready(out, st));
        return guard_bwd_outputs(guard, in, out, 0);
    }
    lsr_settings s2 = *s;
    s2.quick_render = 0;
    s2.quick_dim = 0;
    lsr_inputs in2 = *in;
    in2.quick_k = 0;
    in2.language_feature_weights_quick = nullptr;
    in2.language_feature_indices = nullptr;
    lsr_bwd_out o2 = *out;
    o2.dL_dlang_weights = nullptr;
    o2.lang_ready_event = nullptr;
    lsr_bwd_in b2 = *b;
    float* dense_grad = nullptr;
    if (b->dL_dout_lang) {
        if (lang_set_for(Dq) < 0) return LSR_EUNSUPPORTED;
        const size_t row = (size_t)P * Dq * 4;
        uint8_t* ws = (uint8_t*)alloc(ctx, align256(row) + (dw ? row : 0), LSR_BUF_SPARSE);
        if (!ws) return LSR_ENOMEM;
        float* dense = (float*)ws;
        dense_grad = dw ? (float*)(ws + align256(row)) : nullptr;
        LSR_HIP(launch_sparse_expand(in->language_feature_weights_quick, in->language_feature_indices,
                                     in->quick_index_dtype, P, in->quick_k, Dq, dense, st));
        s2.include_feature = 1;
        in2.lang_dim = Dq;
        in2.language_feature_precomp = dense;
        o2.dL_dlang = dense_grad;
    } else {
        s2.include_feature = 0;
        in2.lang_dim = 0;
        in2.language_feature_precomp = nullptr;
        o2.dL_dlang = nullptr;
        b2.dL_dout_lang = nullptr;
        if (dw) LSR_TRY(zero_weight_grads(in, dw, st));
    }
    // the dense backward shares this call's guard (its flag word stays owned by one Guard)
    LSR_TRY(backward_dense(&s2, &in2, &b2, &o2, alloc, ctx, st, guard));
    if (dw && dense_grad)
        LSR_HIP(launch_sparse_gather(dense_grad, in->language_feature_indices, in->quick_index_dtype, P, in->quick_k,
                                     Dq, dw, st));
    LSR_TRY(record_lang_ready(out, st));
    return guard_bwd_outputs(guard, in, out, 0);
}

}  // namespace

extern "C" {

// preprocess -> bin -> prepare the backward -> render
int lsr_forward(const lsr_settings* s, const lsr_inputs* in, lsr_fwd_out* out, lsr_alloc_fn alloc, void* ctx,
                void* stream)
{
    LSR_TRY(validate(s, in));
    if (!out || !alloc || !out->out_color || (in->P > 0 && !out->radii)) return LSR_EINVAL;
    const int Dd = dense_dim(s, in);
    if ((Dd > 0 || s->quick_render) && !out->out_lang) return LSR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Cam c = make_cam(s);
    const int P = in->P;
    const int T = c.gx * c.gy;
    const size_t NPIX = (size_t)c.W * c.H;

    Guard guard(s, alloc, ctx, st);
    LSR_TRY(guard_inputs(guard, s, in));

    const GeomLayout GL = geom_layout((size_t)P);
    const ImageLayout IL = image_layout(NPIX, (size_t)T);
    const BinShape bs(c, P);
    uint8_t* geom = (uint8_t*)alloc(ctx, GL.total, LSR_BUF_GEOM);
    uint8_t* img = (uint8_t*)alloc(ctx, IL.total + bs.table_bytes, LSR_BUF_IMAGE);
    if (!geom || !img) return LSR_ENOMEM;
    out->geom = geom;
    out->geom_bytes = GL.total;
    out->image = img;
    out->image_bytes = IL.total + bs.table_bytes;

    // 1. preprocess.  Split from 512K Gaussians up: the SH colour pass on a second
    // stream, started behind the geometry pass (measurements: DESIGN §8)
    ColourStream* colour = nullptr;
    if (option(LSR_OPT_SPLIT_PREPROCESS) && !s->debug && P >= kSplitPreMinP && in->shs && !in->colors_precomp)
        colour = colour_stream(st);   // nullptr: the fused preprocess below (same results)
    ColourJoin join{colour, st};   // every return after the launch leaves `st` behind the colour pass
    {
        // a pending geometry gradient: the preprocess also stores the SH colour
        // Jacobian the preprocess backward needs (48 B instead of the 192-B SH row)
        const bool jac = (out->grad_ws_request & LSR_GWS_GEOM) != 0 && !s->quick_render;
        StageScope sc(ST_PRE, st);
        LSR_HIP(launch_preprocess(c, *in, geom, out->radii, jac, st, colour != nullptr,
                                  bs.priv ? (uint64_t*)((uint32_t*)(img + IL.cls_cnt) + LSR_COUNT_WORD) : nullptr));
        if (colour)
            LSR_HIP(launch_preprocess_colour(c, *in, geom, out->radii, jac, st, colour->stream, colour->geom_done,
                                             colour->colour_done));
    }
    LSR_DEBUG_SYNC(s, st, "preprocess");

    // 2. bin: M = out->num_rendered instances in out->binning, sorted per tile
    LSR_TRY(bin_tiles(s, c, P, bs, geom, img, out, alloc, ctx, st));

    // 3. the backward's accumulators and block lists, zeroed / written by the render
    RenderArgs ra = make_render_args(s, in, c, geom, (const uint8_t*)out->binning, img, out->num_rendered);
    LSR_TRY(guard.check_lists("render", ra.point_list, (size_t)out->num_rendered, P, ra.tile_start, (size_t)T));
    ra.out_color = out->out_color;
    ra.out_lang = out->out_lang;
    LSR_TRY(prepare_backward(s, in, Dd, out, ra, alloc, ctx));

    // 4. render
    LSR_HIP(join.wait());   // the SH colours of a split preprocess
    { StageScope sc(ST_RENDER, st); LSR_HIP(launch_render_fwd(ra, st)); }
    // the backward's block order from the lists the render just counted
    if (bwd_order_on(T) && ra.lcount) LSR_HIP(launch_bwd_order(ra, (uint4*)(img + IL.border), st));
    LSR_DEBUG_SYNC(s, st, "render");
    LSR_GUARD(guard, "out_color", out->out_color, 3 * NPIX);
    LSR_GUARD(guard, "out_lang", out->out_lang, (size_t)(s->quick_render ? quick_dim(s) : Dd) * NPIX);
    return LSR_OK;
}

int lsr_backward(const lsr_settings* s, const lsr_inputs* in, const lsr_bwd_in* b, lsr_bwd_out* out,
                 lsr_alloc_fn alloc, void* ctx, void* stream)
{
    LSR_TRY(validate(s, in));
    if (!b || !out || !alloc || !b->geom || !b->image || !b->binning || !b->dL_dout_color) return LSR_EINVAL;
    const int Dd = dense_dim(s, in);
    if (Dd > 0 && !b->dL_dout_lang) return LSR_EINVAL;
    if (out->dL_dlang_weights && !s->quick_render) return LSR_EINVAL;
    if (s->quick_render && out->dL_dlang) return LSR_EINVAL;   // the quick input has no dense rows
    if (in->P == 0) return LSR_OK;
    if (!b->radii) return LSR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Cam c = make_cam(s);
    const int P = in->P;
    const size_t NPIX = (size_t)c.W * c.H;
    Guard guard(s, alloc, ctx, st);
    LSR_GUARD(guard, "dL_dout_color", b->dL_dout_color, 3 * NPIX);
    LSR_GUARD(guard, "dL_dout_lang", b->dL_dout_lang, (size_t)(s->quick_render ? quick_dim(s) : Dd) * NPIX);
    if (s->debug) {   // the saved lists the render backward gathers through
        const RenderArgs la = make_render_args(s, in, c, (const uint8_t*)b->geom, (const uint8_t*)b->binning,
                                               (const uint8_t*)b->image, b->num_rendered);
        LSR_TRY(guard.check_lists("render_bwd", la.point_list, (size_t)b->num_rendered, P, la.tile_start,
                                  (size_t)c.gx * c.gy));
    }
    if (s->quick_render) return backward_quick(s, in, b, out, alloc, ctx, st, guard);
    return backward_dense(s, in, b, out, alloc, ctx, st, guard);
}

}  // extern "C"
