// lsr_internal.h — launcher declarations shared by the kernel translation
// units and the C-ABI driver (lsr_api.hip: forward and backward; lsr_api_ops.hip:
// the single-kernel entry points; lsr_api_runtime.hip: options, profiling,
// streams; their shared macros, profiler and guard: lsr_api_common.h).  Not part
// of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lsr.h"
#include "lsr_device.h"

#include <type_traits>

namespace lsr {

// Host dispatch: the launchers pick a kernel instantiation from runtime values
// (the render's integer helpers: render_common.h).
// f(std::bool_constant<b>...) for the runtime bools b...
template <class F>
void with_bools(F&& f)
{
    f();
}
template <class F, class... Bs>
void with_bools(F&& f, bool b, Bs... rest)
{
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

struct Cam {
    int W, H, gx, gy;
    float tanfovx, tanfovy, fx, fy, scale_modifier;
    const float* view;
    const float* proj;
    const float* campos;
    const float* bg;
    int sh_degree;
};

// preprocess.hip
// geom_only (SH inputs): the geometry pass only; the SH colour pass is
// launch_preprocess_colour, on a second stream (lsr_api.hip, split preprocess)
hipError_t launch_preprocess(const Cam& c, const lsr_inputs& in, uint8_t* geom, int32_t* radii, bool jac,
                             hipStream_t st, bool geom_only = false, uint64_t* zero_word = nullptr);
hipError_t launch_preprocess_colour(const Cam& c, const lsr_inputs& in, uint8_t* geom, const int32_t* radii, bool jac,
                                    hipStream_t st, hipStream_t colour_st, hipEvent_t ready, hipEvent_t done);
hipError_t launch_sh_grad_from_views(int64_t N, int M, int deg, const float* means3D, int R, const float* campos,
                                     const float* drgb, float* dL_dsh, hipStream_t st);
hipError_t launch_preprocess_bwd(const Cam& c, const lsr_inputs& in, const uint8_t* geom, const int32_t* radii,
                                 const float* grad_acc, int VP, const lsr_bwd_out& out, hipStream_t st);
hipError_t launch_mark_visible(int P, const float* means, const float* view, uint8_t* present, hipStream_t st);

// scan.hip
// Inclusive scan of n uint32 values (in-place allowed); writes the 64-bit total
// to part[0] (part must hold scan_partials(n) uint64 entries).
size_t scan_partials(size_t n);
hipError_t launch_scan_u32(const uint32_t* in, uint32_t* out, uint64_t* part, size_t n, bool exclusive, hipStream_t st);

// binning.hip
// The binning's arrays in the image workspace and the privatised path's shape
// (lsr_api.hip bin_tiles fills it once; T = gx gy tiles).
struct BinWs {
    int chunk, B;           // Gaussians per count chunk, chunks (bin_blocks; B >= 1 on the privatised path)
    uint32_t* table;        // B x table_stride(T): per-chunk tile counts, then the chunks' bases
    uint32_t* tile_cnt;     // T
    uint32_t* tile_start;   // T + 1
    uint64_t* tpart;        // the tile scan's partials / the 64-tile groups' bases
    uint32_t* cls_cnt;      // SORT_NCLS class counts, LSR_TICKET_WORD, LSR_COUNT_WORD
    uint32_t* cls_list;     // SORT_NCLS x T: the classes' tiles
};
// The coherent pinned host line M is published to (device view), with the
// forward's sequence number (lsr_api.hip HostSlot).
struct HostWord {
    uint64_t* dev;
    uint32_t seq;
};
#define LSR_TICKET_WORD 32   // cls_cnt word k_bin_table counts arrivals in (own 128-B line)
#define LSR_COUNT_WORD 64    // cls_cnt words (one u64) k_bin_count sums M and arrivals in (own line;
                             // zeroed by the preprocess)
#define LSR_CLS_SLOT 4       // pinned host word (u64 index) k_bin_table publishes the class counts under
                             // (the counts themselves: u32 words 2 .. 1 + SORT_NCLS of the line)
hipError_t launch_publish_total(const uint64_t* total, const HostWord& hw, hipStream_t st);
hipError_t launch_duplicate(const Cam& c, int P, const uint8_t* geom, const int32_t* radii, uint32_t* tile_cnt,
                            uint32_t* rank, hipStream_t st);
hipError_t launch_scatter(const Cam& c, int P, const uint8_t* geom, const int32_t* radii, const uint32_t* tile_start,
                          const uint32_t* rank, uint64_t* keys, hipStream_t st);
int bin_blocks(int P, const Cam& c, int& chunk);
bool bin_privatised_ok(const Cam& c);
// count + column scan + group-level tile scan; publishes M (word 0) and then
// M with the sort class counts (word LSR_CLS_SLOT) to the host line
hipError_t launch_bin_count(const Cam& c, int P, const uint8_t* geom, const int32_t* radii, const BinWs& ws,
                            const HostWord& hw, hipStream_t st);
int bin_scatter_rows(const Cam& c);
int scatter_merge(int P);
int bin_block(int P);
// tile_start[0..T) from tile_cnt and the group bases launch_bin_count left in tpart
hipError_t launch_tile_start_apply(int T, const BinWs& ws, hipStream_t st);
hipError_t launch_bin_scatter(const Cam& c, int P, const uint8_t* geom, const int32_t* radii, const BinWs& ws,
                              uint64_t* keys, hipStream_t st);

// tile_sort.hip
// Tile-sort size classes (tile_sort.h tile_class); their per-class tile counts
// and lists live in the image workspace (BinWs::cls_cnt, cls_list).
#define SORT_NCLS 5
// host_cnt: the per-class tile counts when the host already has them (the
// privatised binning path publishes them with M); null = unknown, the lists
// are built here and every class runs a persistent grid.
hipError_t launch_tile_sort(int T, const BinWs& ws, uint64_t* keys, uint32_t* point_list, const uint32_t* host_cnt,
                            hipStream_t st);


// render_fwd.hip, render_quick.hip (the forward render; RenderArgs is also the
// backward's view of the forward, RenderBwdArgs::f)
struct RenderArgs {
    Cam cam;
    int P;
    const float4* splatA;
    const float4* splatB;
    const float* rgb;            // (P,3): preprocess output or colors_precomp
    const float* lang;           // (P,D) dense or NULL
    int D;                       // dense language channels rendered (0 if off)
    const float* qw;             // quick weights (P,K) or NULL
    const void* qi;              // quick indices (P,K)
    int qidx_dtype, K, Dq;
    int quick_hwc;   // out_lang pixel-major (H, W, Dq) (lsr_settings.quick_layout)
    const uint32_t* point_list;
    const uint32_t* tile_start;  // T+1
    float* final_T;
    uint32_t* n_contrib;
    float* out_color;
    float* out_lang;
    // the backward's accumulators, zeroed by the dense forward render (NULL: none)
    float4* zero = nullptr;
    size_t zero_n16 = 0;
    float4* zero2 = nullptr;   // the (N, D) dL/dlang accumulator (its own allocation)
    size_t zero2_n16 = 0;
    // per-8x8-block candidate lists for the backward (lsr_fwd_out.lists; NULL: none).
    // Block b = 4 tile + sub owns entries [4 tile_start[tile] + sub n_tile, + n_tile)
    // of listA / listB (n_tile = the tile's instance count); lcount[b] = its entries
    // below the block's largest n_contrib (an over-count is harmless)
    float4* listA = nullptr;   // the candidate's splat record A {x, y, conic.a, conic.b}
    float4* listB = nullptr;   // {conic.c, opacity, id bits, 0-based tile-list position bits}
    uint32_t* lcount = nullptr;
    // backward only: the blocks in dispatch order, heaviest list first inside
    // each XCD's range (k_bwd_order; null = band order)
    const uint4* border = nullptr;   // {block 4 tile + sub, tile_start[tile], tile_start[tile + 1], lcount[block]}
};
hipError_t launch_render_fwd(const RenderArgs& a, hipStream_t st);
// its quick arm (a.qw set, at least one tile): render_quick.hip
hipError_t launch_render_fwd_quick(const RenderArgs& a, hipStream_t st);
int lang_set_for(int D);     // compiled channel set >= D, or -1

// render_bwd.hip
// the backward's block order (RenderArgs::border, 4 T entries) from the forward's lcount
#ifndef LSR_BWD_ORDER
#define LSR_BWD_ORDER 1   // list-driven backward: heaviest block lists dispatched first (0: band order)
#endif
// from this many 8x8 blocks (4 T) up: four or more generations of the
// backward's 4,096 resident waves, where its drain is worth the order
// kernel's ~7.5 us (cfg3: 32,640 blocks)
#define LSR_BWD_ORDER_MIN_BLOCKS 16384
inline bool bwd_order_on(int T) { return LSR_BWD_ORDER && 4 * (int64_t)T >= LSR_BWD_ORDER_MIN_BLOCKS; }
hipError_t launch_bwd_order(const RenderArgs& a, uint4* border, hipStream_t st);

struct RenderBwdArgs {
    RenderArgs f;
    const float* dout_color;
    const float* dout_lang;
    float* grad_acc;   // (P, VP) atomically accumulated
    int VP;
    // non-null: dL/dlanguage is accumulated straight into this (P, D) output
    // (zeroed by the caller) and the gradient rows hold geometry + colour only
    float* lang_acc = nullptr;
    // non-null (language-only backward in quick mode): dL/dweights (P, K) of
    // the sparse input f.qw / f.qi, accumulated with the channel gradient
    // gathered at each Gaussian's codes (zeroed by the caller)
    float* qw_acc = nullptr;
    // LSR_OPT_DETERMINISTIC: the atomics add 64-bit fixed-point twins of grad_acc
    // (det_rows, same (P, VP) indexing) and lang_acc (det_lang, (P, D)), each value
    // scaled by 2^det_shift(...) (render_det.h); det_bounds = {max |dL/dout|,
    // max |feature|, flag bits} from launch_det_bounds, radii the forward's
    long long* det_rows = nullptr;
    long long* det_lang = nullptr;
    float* det_bounds = nullptr;
    const int32_t* radii = nullptr;
    // per Gaussian, the four column classes' shifts as signed bytes (class k in
    // byte k), written by launch_det_bounds and read by the adds and the
    // conversion alike
    uint32_t* det_sh = nullptr;
};
bool bwd_lang_direct(int D);  // D for which the full backward supports lang_acc
int grad_row_width(int D);   // VP for a dense language dim
hipError_t launch_render_bwd(const RenderBwdArgs& a, hipStream_t st);
// language-only backward: grad_acc is the (P, D) dL/dlanguage output itself
// (zeroed by the caller), VP = D
hipError_t launch_render_bwd_lang(const RenderBwdArgs& a, hipStream_t st);
// language-only backward of the quick (sparse) input: a.qw_acc (P, K) from
// the Dq-channel gradient (Dq must be a compiled channel set, <= 64)
hipError_t launch_render_bwd_lang_sparse(const RenderBwdArgs& a, hipStream_t st);

// render_det.hip
// LSR_OPT_DETERMINISTIC: bounds = {max |dL/dout| over the 3 + D planes,
// max |feature| over the visible Gaussians' colours and the dense language input,
// flag} (flag bit 0: a non-finite value).  bounds points at LSR_DET_HDR bytes:
// the 3 words, then the per-block partials (every word written, no atomics)
constexpr int LSR_DET_BLOCKS = 32768;
constexpr size_t LSR_DET_HDR = 256 + 3 * 4 * LSR_DET_BLOCKS;
hipError_t launch_det_bounds(const RenderBwdArgs& b, float* bounds, hipStream_t st);
// the fixed-point sums back to fp32: rows (P, VP) -> grad_out (every element
// written; VP = 16 with lang_direct), lang (P, D) -> lang_out; lang_only: rows
// is the (P, D) language accumulator and lang_out its output.  A flagged
// bounds word writes NaN everywhere.
hipError_t launch_det_finish(const RenderBwdArgs& b, bool lang_only, float* grad_out, float* lang_out,
                             hipStream_t st);

// lang_codes.hip
hipError_t launch_topk_code_fwd(const float* logits, int64_t N, int L, int K, int k, float* dense, float* sw,
                                void* sidx, int idx_dtype, int level_offset, hipStream_t st);
// sparse: g is dL/dweights of the packed (N, L*k) form (ascending channel order)
hipError_t launch_topk_code_bwd(const float* logits, const float* g, int64_t N, int L, int K, int k, float* dlogits,
                                hipStream_t st, bool sparse = false);
// knn.hip
size_t knn_workspace_bytes(int64_t N, size_t sort_temp);
hipError_t knn_sort_temp_bytes(int64_t N, size_t* bytes);
hipError_t launch_knn_dist2(const float* points, int64_t N, float* out, uint8_t* ws, size_t sort_temp, hipStream_t st);

// quick_decode.hip: codebook decode of the quick language map (K = 64, Df % 16 == 0)
size_t quick_decode_workspace_bytes(int L, int K, int Df, int normalize);
hipError_t launch_quick_decode_prepare(const float* cb, int L, int K, int Df, int normalize, void* ws, hipStream_t st);
hipError_t launch_quick_decode_run(const float* wmap, int L, int K, int Df, int H, int W, int normalize, float eps,
                                   const void* ws, float* out, hipStream_t st, bool hwc = false);
hipError_t launch_quick_decode(const float* wmap, const float* cb, int L, int K, int Df, int H, int W, int normalize,
                               float eps, void* ws, float* out, hipStream_t st);
// the plan pieces the query plan shares: split-f16 fragments + per-level scales of
// (L, K, Df) matrices, and the norm factor of every level: Gram matrix G (L, K, K)
// -> its Cholesky factor Lf (L, K, K) -> the factor's fragments + scales (chol),
// or the Gram matrices' own fragments (!chol)
void launch_codebook_frag(const float* cb, int L, int K, int Df, uint4* frag, float* scales, hipStream_t st);
void norm_factor_prepare(const float* cb, int L, int K, int Df, float* G, float* Lf, uint4* nfrag, float* nscales,
                         bool chol, hipStream_t st);

// quick_query.hip: fused text-query relevancy / cosine maps (K = 64, n_pos + n_neg <= 64)
size_t quick_query_plan_bytes(int L, int K, int n_pos, int n_neg);
hipError_t launch_quick_query_prepare(const float* cb, const float* pos, const float* neg, int L, int K, int Df,
                                      int n_pos, int n_neg, void* ws, hipStream_t st);
hipError_t launch_quick_query_run(const float* wmap, bool hwc, const void* ws, int L, int K, int n_pos, int n_neg,
                                  int H, int W, bool relevancy, float scale, float eps, float* out, hipStream_t st);
// the f32 projections P (L, K, ncp) = CB_l E^T the heat and semantic plans share: columns = the negatives, the
// positives, zeros
void launch_query_project(const float* cb, const float* pos, const float* neg, int L, int K, int Df, int n_pos,
                          int n_neg, int ncp, float* P, hipStream_t st);

// quick_semantic.hip: fused label maps (K = 64, n_lab + n_neg <= 256; columns: the labels, then the negatives;
// scores == nullptr: labels only), their level merge and the confusion counts of an evaluation
size_t quick_semantic_plan_bytes(int L, int K, int n_lab, int n_neg);
hipError_t launch_quick_semantic_prepare(const float* cb, const float* lab, const float* neg, int L, int K, int Df,
                                         int n_lab, int n_neg, void* ws, hipStream_t st);
hipError_t launch_quick_semantic_run(const float* wmap, bool hwc, const void* ws, int L, int K, int n_lab, int n_neg,
                                     int H, int W, float scale, float eps, int32_t* labels, float* scores,
                                     hipStream_t st);
hipError_t launch_semantic_merge(const int32_t* labels, const float* scores, int L, int H, int W, int32_t* out,
                                 uint8_t* level, hipStream_t st);
// counts (P, C, C + 1) int64, zeroed here
hipError_t launch_semantic_confusion(const int32_t* pred, const int32_t* gt, int P, int H, int W, int C,
                                     int64_t* counts, hipStream_t st);

// quick_heat.hip: the viewer's maps (summed-level cosine / mean relevancy, (n_pos, H, W); K = 64, L <= 3,
// n_pos + n_neg <= 64) and the colour stage (gate, curve, table, blend with rgb, uint8 (planes, H, W, 3))
size_t quick_heat_plan_bytes(int L, int K, int n_pos, int n_neg);
hipError_t launch_quick_heat_prepare(const float* cb, const float* pos, const float* neg, int L, int K, int Df,
                                     int n_pos, int n_neg, void* ws, hipStream_t st);
hipError_t launch_quick_heat_run(const float* wmap, bool hwc, const void* ws, int L, int K, int n_pos, int n_neg,
                                 int H, int W, bool mean, float scale, float eps, float* out, hipStream_t st);
bool heat_frame_shape_ok(int planes, int H, int W);
hipError_t launch_heat_frame(const float* maps, const float* stats, const float* rgb, const uint8_t* lut, int planes,
                             int H, int W, bool power4, float threshold, float min_range, float alpha, uint8_t* out,
                             hipStream_t st);

// query_post.hip: smoothing, masks and localisation of (planes, H, W) relevancy maps
bool query_post_shape_ok(int planes, int H, int W);
size_t query_post_workspace_bytes(int planes, int H, int W);
// box mean of radius r (avg, blend optional), then per plane stats (planes, 3) =
// {min blend, max blend, max avg} and loc (planes, 2) = {first row-major pixel of max avg, ties}
hipError_t launch_query_smooth(const float* rel, int planes, int H, int W, int r, float* avg, float* blend,
                               float* stats, int64_t* loc, void* ws, hipStream_t st);
// thresholded, majority-smoothed (radius s) masks of blend normalised by stats; counts (planes, 3) =
// {area, intersection, union with gt[plane % n_prompt] (0 without gt)}, masked_sum (planes)
hipError_t launch_query_mask(const float* blend, const float* stats, const uint8_t* gt, int planes, int n_prompt,
                             int H, int W, float thresh, int s, uint8_t* mask, int64_t* counts, float* masked_sum,
                             void* ws, hipStream_t st);

// lang_loss.hip
size_t lang_loss_workspace_bytes(int S, int W, int H, int* waves);
// gw == nullptr: forward (loss and/or the per-pixel stats (2, H, W));
// else dL/dweight_map and dL/dcodebooks scaled by *gscale, from the
// forward's stats (recomputed when stats == nullptr)
hipError_t launch_lang_loss(const float* wmap, const float* cb, int Df, int H, int W, const int32_t* seg,
                            const float* feat, int S, const float* gscale, float* loss, float* gw, float* dcb,
                            float* stats, float* ws, hipStream_t st);

// lang_loss.hip, the L1 pair (--l1_loss, optionally --normalize): normalize != 0 divides f_p by |f_p| + 1e-10
size_t lang_l1_workspace_bytes(int Df, int W, int H);
// gw == nullptr: forward (loss and, with normalize, the per-pixel stats (2, H, W) = |f_p|, sum_d u_pd sign_pd);
// else dL/dweight_map and dL/dcodebooks scaled by *gscale, from the forward's stats (recomputed when nullptr)
hipError_t launch_lang_l1(const float* wmap, const float* cb, int Df, int H, int W, const int32_t* seg,
                          const float* feat, int S, int normalize, const float* gscale, float* loss, float* gw,
                          float* dcb, float* stats, float* ws, hipStream_t st);

// photo_loss.hip: L1 + SSIM of (planes, H, W) images (planes H W < 2^31)
struct PhotoTaps {
    float w[11];   // the normalised 1-D window (sigma 1.5), formed in double and rounded once
};
size_t photo_loss_workspace_bytes(int planes, int H, int W);
// out[0] = mean |x - y|, out[1] = mean SSIM; partials (3, planes, H, W) or nullptr
hipError_t launch_photo_loss_fwd(const float* x, const float* y, int planes, int H, int W, const PhotoTaps& tp,
                                 float* out, float* partials, void* ws, hipStream_t st);
// gx = g[0] dL1/dx + g[1] dSSIM/dx from the forward's partials (g: device float[2])
hipError_t launch_photo_loss_bwd(const float* x, const float* y, int planes, int H, int W, const PhotoTaps& tp,
                                 const float* partials, const float* g, float* gx, hipStream_t st);

// kmeans.hip: Lloyd's iteration over an (M, D) feature table (D % 4 == 0, 4 <= D <= 1024, 1 <= K <= 256, M < 2^31)
size_t kmeans_workspace_bytes(int64_t M, int K, int D);
// the centres' MFMA fragments, norms and raw copy into ws (once per centre set)
hipError_t launch_kmeans_prepare(const float* centers, int K, int D, void* ws, hipStream_t st);
// assign (M) = nearest prepared centre, ties to the lowest index; dist (M) = max(|x - c|^2, 0);
// residual (M, D) = x - c[assign] or nullptr (must not alias x)
hipError_t launch_kmeans_assign(const float* x, int M, int D, int K, const void* ws, int* assign, float* dist,
                                float* residual, hipStream_t st);
// centers_out (K, D) = per-cluster means (an empty cluster: its prepared centre), counts_out (K);
// then prepares centers_out in ws
hipError_t launch_kmeans_update(const float* x, const int* assign, int M, int D, int K, void* ws, float* centers_out,
                                int* counts_out, hipStream_t st);

// mask_nms.hip: SAM mask NMS and segment maps on bit-packed masks (N <= LSR_MASK_MAX_N, HW <= LSR_MASK_MAX_PIXELS)
size_t mask_nms_workspace_bytes(int N);   // starts with the (N, N) int32 pair table
hipError_t launch_mask_pack(const uint8_t* masks, int N, int HW, unsigned long long* words, int* area, hipStream_t st);
// inter (N, N): |mask order[i] & mask order[j]| for i <= j, 0 below the diagonal
hipError_t launch_mask_pairs(const unsigned long long* words, int N, int W64, const int* order, int* inter,
                             hipStream_t st);
// from the pair table at the start of ws: keep, criteria (or nullptr), selected, count
hipError_t launch_mask_decide(const int* area, int N, const int* order, const uint8_t* conf, float iou_thr,
                              float inner_cut, void* ws, uint8_t* keep, uint8_t* criteria, long long* selected,
                              int* count, hipStream_t st);
// out (4, HW) as int32 or fp32; the five arrays are host arrays of 4
hipError_t launch_mask_segmaps(const unsigned long long* const* words, const int* const* kept, const int* masks,
                               const int* counts, const int* offsets, int HW, bool as_int, void* out, hipStream_t st);

// clip_tiles.hip: tight boxes of packed masks; the S x S CLIP tiles of n of them (S <= LSR_TILE_MAX_SIDE)
hipError_t launch_mask_boxes(const unsigned long long* words, int N, int H, int W, int* boxes, hipStream_t st);
// out: (n, S, S, 3) uint8 (LSR_TILE_U8) or (n, 3, S, S) through lut (3, 256), fp32 (_UNIT) or fp16 (_CLIP)
hipError_t launch_clip_tiles(const uint8_t* image, int H, int W, const unsigned long long* words, int N,
                             const int* keep, const int* boxes, int n, int S, const void* lut, int out_type, void* out,
                             hipStream_t st);

// densify.hip: densify_and_prune as one gather (plan: classify, scan, fill; apply: all 18 tensors)
struct DensifyArgs {
    float max_grad, dense_thresh, min_opacity, big_thresh;   // thresholds as the reference's fp32 comparisons see them
    int prune_big;                                           // max_screen_size truthy
};
struct DensifyTable {   // entry part * LSR_DENSIFY_GROUPS + group; part 0 parameter, 1 exp_avg, 2 exp_avg_sq
    const float* src[3 * LSR_DENSIFY_GROUPS];
    float* dst[3 * LSR_DENSIFY_GROUPS];   // nullptr: skipped
    int width[LSR_DENSIFY_GROUPS];
    const float* noise;                   // (N, 2, 3)
};
size_t densify_workspace_bytes(int64_t N);
hipError_t launch_densify_plan(int64_t N, const float* accum, const float* denom, const float* scaling,
                               const float* opacity, const DensifyArgs& a, void* ws, hipStream_t st);
const int64_t* densify_counts(int64_t N, const void* ws);   // device int64[LSR_DENSIFY_COUNTS] inside ws
hipError_t launch_densify_apply(int64_t N, int64_t n_out, const void* ws, const DensifyTable& t, hipStream_t st);
hipError_t launch_reset_opacity(int64_t n, float* opacity, float* m, float* v, hipStream_t st);

// aux.hip: debug NaN/Inf guard (flag |= 1 if any element of p[0..n) is not
// finite) and the quick-input dense expansion / gradient gather
hipError_t launch_nonfinite(const float* p, size_t n, uint32_t* flag, hipStream_t st);
hipError_t launch_check_lists(const uint32_t* point_list, size_t M, uint32_t P, const uint32_t* tile_start, size_t T,
                              uint32_t* flag, hipStream_t st);
hipError_t launch_sparse_expand(const float* qw, const void* qi, int dtype, int N, int K, int Dq, float* dense,
                                hipStream_t st);
hipError_t launch_sparse_gather(const float* g, const void* qi, int dtype, int N, int K, int Dq, float* dw,
                                hipStream_t st);
hipError_t launch_quick_pack_codes(const void* qi, int dtype, int64_t N, int Dq, void* packed, hipStream_t st);

// adam.hip
struct AdamArgs {
    float one_minus_b1, b2, one_minus_b2, eps, step_size, bc2_sqrt, weight_decay;
};
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, const AdamArgs& a, hipStream_t st);

}  // namespace lsr
