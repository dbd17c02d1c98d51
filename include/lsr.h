/*
 * lsr.h — C ABI of the MI355X-native language-Gaussian tile rasterizer
 * (liblsr.so, hand-written HIP for gfx950).
 *
 * This is the drop-in boundary under the reference's operator surface
 * `diff_gaussian_rasterization` (imported at gaussian_renderer/__init__.py:15,
 * constructed :37-54, called :108-119).  Each entry point replaces one
 * binding of the reference's (absent) torch extension `_C`
 * (submodules/efficient-langsplat-rasterization, .gitmodules:1-3):
 *
 *   lsr_forward      <- _C.rasterize_gaussians           (forward of
 *                       GaussianRasterizer.__call__, gaussian_renderer/__init__.py:108-119)
 *   lsr_backward     <- _C.rasterize_gaussians_backward  (autograd backward,
 *                       reached from loss.backward() at train.py:173)
 *   lsr_mark_visible <- _C.mark_visible                  (GaussianRasterizer.markVisible)
 *   lsr_strerror     <- the RuntimeError text the binding raises
 *
 * Conventions
 *  - All tensor pointers are DEVICE pointers to contiguous fp32 (int32 for
 *    radii) arrays with the shapes documented per field; optional inputs are
 *    NULL.  N = number of Gaussians, H×W image, D dense language channels,
 *    K quick entries per Gaussian, Dq quick output channels.
 *  - Matrices are the reference's `world_view_transform` /
 *    `full_proj_transform` tensors as stored (row-major transposed, i.e.
 *    column-major math matrices; scene/cameras.py:55-57).
 *  - The library never allocates device memory itself: workspaces are
 *    requested through `alloc(ctx, bytes, which)` (torch's caching allocator
 *    on the Python side) and returned in the out struct so the caller can
 *    keep them for backward (the upstream geomBuffer/binningBuffer/imgBuffer
 *    pattern).  Returned pointers must be 256-byte aligned.
 *  - All work is enqueued on `stream` (a hipStream_t).  lsr_forward performs
 *    exactly one host synchronisation (the num_rendered read-back that sizes
 *    the binning workspace).
 *  - Return value 0 = success; otherwise an LSR_E* code (lsr_strerror).
 */
#ifndef LSR_H
#define LSR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_ABI_VERSION 12  /* 12, additive (no bump): lsr_quick_semantic_plan_bytes / _prepare / _run, lsr_semantic_merge / _confusion;
                               12, additive (no bump): lsr_mask_boxes, lsr_clip_tiles;
                               12, additive (no bump): lsr_mask_nms_workspace_bytes, lsr_mask_pack / _pair_counts / _nms_select / _segmaps;
                               12, additive (no bump): lsr_kmeans_workspace_bytes / _prepare / _assign / _update;
                               12, additive (no bump): lsr_photo_loss_forward / _backward;
                               12, additive (no bump): lsr_quick_heat_plan_bytes / _prepare / _run, lsr_heat_frame;
                               12, additive (no bump): lsr_query_post_workspace_bytes, lsr_query_smooth, lsr_query_mask;
                               12, additive (no bump): lsr_quick_query_plan_bytes / _prepare / _run;
                               12 (r06): LSR_OPT_DETERMINISTIC;
                               11 (r05): LSR_INDEX_PACKED, lsr_quick_pack_codes, LSR_OPT_SPLIT_PREPROCESS;
                               10 (r05): lsr_settings.quick_layout, lsr_quick_decode_run weight_layout;
                               9 (r05): LSR_OPT_LISTS_MAX_MB; LSR_BIN_ORDERED removed */

enum {
    LSR_OK = 0,
    LSR_EINVAL = 1,        /* invalid argument / shape / missing input */
    LSR_EUNSUPPORTED = 2,  /* e.g. language dim beyond the compiled channel sets */
    LSR_EHIP = 3,          /* HIP launch / runtime failure */
    LSR_ENOMEM = 4,        /* alloc callback returned NULL */
    LSR_EOVERFLOW = 5,     /* num_rendered does not fit 32-bit instance indices */
    LSR_ENONFINITE = 6,    /* debug guard: NaN/Inf in an input or output */
    LSR_ELISTS = 7         /* debug check: corrupt binning lists (id >= P, tile ranges not monotone) */
};

/* GaussianRasterizationSettings (gaussian_renderer/__init__.py:37-52),
 * field for field, plus the optional trailing quick_dim (u4). */
typedef struct lsr_settings {
    int image_height;
    int image_width;
    float tanfovx;
    float tanfovy;
    const float* bg;          /* (3,) device */
    float scale_modifier;
    const float* viewmatrix;  /* (4,4) device */
    const float* projmatrix;  /* (4,4) device */
    int sh_degree;            /* active SH degree (0..3) */
    const float* campos;      /* (3,) device */
    int prefiltered;
    int debug;                /* sync + check after every stage */
    int include_feature;      /* dense language channels on */
    int quick_render;         /* sparse (weights, indices) language channels on */
    int quick_dim;            /* Dq; 0 selects the reference default 192 */
    int quick_layout;         /* LSR_LAYOUT_CHW (0, the reference's (Dq,H,W)) or LSR_LAYOUT_HWC:
                                 out_lang is written pixel-major, (H,W,Dq) — every pixel's Dq
                                 weights in one 768-B row at Dq = 192 (the quick_render kernel
                                 with K = 12, Dq = 192 only; else LSR_EUNSUPPORTED) */
} lsr_settings;

enum { LSR_LAYOUT_CHW = 0, LSR_LAYOUT_HWC = 1 };

/* Code-index dtypes of language_feature_indices.  LSR_INDEX_PACKED: an (N, 4)
 * uint32 array written by lsr_quick_pack_codes (K = 12 codes per Gaussian as
 * bytes code + 1, 0 = no code, 16-B rows): what the quick render stages per
 * candidate, so a caller rendering many views of one model converts the
 * reference's fp32 indices once instead of every frame.  Forward and backward
 * of quick_render with K = 12, Dq <= 192 and 16-B aligned weights / indices
 * only (else LSR_EUNSUPPORTED); bytes above Dq are dropped as out-of-range
 * codes are. */
enum { LSR_INDEX_F32 = 0, LSR_INDEX_I32 = 1, LSR_INDEX_I64 = 2, LSR_INDEX_PACKED = 3 };

/* GaussianRasterizer.forward kwargs (gaussian_renderer/__init__.py:108-119). */
typedef struct lsr_inputs {
    int P;                          /* N */
    int max_coeffs;                 /* shs.shape[1] (16 at degree 3) */
    int lang_dim;                   /* D = language_feature_precomp.shape[1] */
    int quick_k;                    /* K = language_feature_weights_quick.shape[1] */
    int quick_index_dtype;          /* LSR_INDEX_* of language_feature_indices */
    const float* means3D;           /* (N,3) */
    const float* shs;               /* (N,M,3) or NULL */
    const float* colors_precomp;    /* (N,3) or NULL (exactly one of shs/colors) */
    const float* opacities;         /* (N,1) */
    const float* scales;            /* (N,3) or NULL */
    const float* rotations;         /* (N,4) wxyz or NULL (normalised by caller) */
    const float* cov3D_precomp;     /* (N,6) or NULL (exactly one of scale+rot/cov) */
    const float* language_feature_precomp;       /* (N,D) or NULL */
    const float* language_feature_weights_quick; /* (N,K) or NULL */
    const void* language_feature_indices;        /* (N,K) or NULL */
} lsr_inputs;

/* Workspace allocator.  lsr_forward may request LSR_BUF_BINNING twice in
 * one call: a speculative buffer sized from the previous call's M (taken
 * while the GPU is still counting) and, only if M outgrew it, a second one;
 * the last pointer returned for a kind is the one the call uses. */
typedef void* (*lsr_alloc_fn)(void* ctx, size_t bytes, int which);
enum { LSR_BUF_GEOM = 0, LSR_BUF_BINNING = 1, LSR_BUF_IMAGE = 2, LSR_BUF_GRAD = 3, LSR_BUF_DECODE = 4,
       LSR_BUF_KNN = 5, LSR_BUF_LOSS = 6, LSR_BUF_GUARD = 7, LSR_BUF_SPARSE = 8, LSR_BUF_GRAD_LANG = 9,
       LSR_BUF_LISTS = 10, LSR_BUF_DET = 11 /* LSR_OPT_DETERMINISTIC: bounds + fixed-point accumulators */ };

typedef struct lsr_fwd_out {
    float* out_color;     /* (3,H,W)  caller-allocated */
    float* out_lang;      /* (Dout,H,W) caller-allocated, Dout = D (dense), Dq (quick) or 0 */
    int32_t* radii;       /* (N,) caller-allocated */
    /* filled by lsr_forward: */
    void* geom;    size_t geom_bytes;
    void* binning; size_t binning_bytes;   /* capacity (>= layout for num_rendered) */
    void* image;   size_t image_bytes;
    int64_t num_rendered;
    /* Optional: the backward's accumulators, prepared by the forward.  In:
     * grad_ws_request = LSR_GWS_GEOM (the backward will request geometry /
     * colour gradients) | LSR_GWS_LANG (it will request dL_dlang).  The
     * forward then allocates them and zeroes them inside the render kernel
     * instead of the backward clearing them with memsets; out: grad_ws /
     * grad_ws_bytes (the gradient rows, LSR_BUF_GRAD; NULL when only dL/dlang
     * is requested), grad_ws_lang (an (N,D) dL/dlang accumulator in its OWN
     * allocation, LSR_BUF_GRAD_LANG, so the gradient returned from it keeps
     * nothing else alive; NULL: none) and grad_ws_kind.
     * Dense language path only (quick_render: nothing prepared). */
    int grad_ws_request;
    int grad_ws_kind;
    void* grad_ws; size_t grad_ws_bytes; void* grad_ws_lang;
    /* With grad_ws_request set (dense path), also: each 8x8 block's candidate
     * list for the backward (LSR_BUF_LISTS; NULL when not prepared), written by
     * the render: pass it in lsr_bwd_in.lists to let the backward read its
     * candidates instead of re-staging them from the tile lists. */
    void* lists; size_t lists_bytes;
} lsr_fwd_out;
enum { LSR_GWS_GEOM = 1, LSR_GWS_LANG = 2 };

/* _C.rasterize_gaussians: preprocess → binning (tile buckets + per-tile depth
 * sort) → per-pixel alpha blend of RGB + language channels.  With
 * settings.debug set, inputs and outputs are also scanned for NaN/Inf
 * (LSR_ENONFINITE). */
int lsr_forward(const lsr_settings* s, const lsr_inputs* in, lsr_fwd_out* out,
                lsr_alloc_fn alloc, void* alloc_ctx, void* stream);

typedef struct lsr_bwd_in {
    const void* geom;
    const void* binning;
    const void* image;
    int64_t num_rendered;
    const int32_t* radii;           /* (N,) from forward */
    const float* dL_dout_color;     /* (3,H,W) */
    const float* dL_dout_lang;      /* (D,H,W) or NULL */
    /* Optional: lsr_fwd_out.grad_ws / _bytes / _kind / _lang of the same
     * forward (zeroed accumulators; hand them to ONE backward).  Used when the
     * kind matches what this call's requested outputs need (otherwise the call
     * allocates and clears its own); dL_dlang == grad_ws_lang then needs no
     * clearing either. */
    void* grad_ws; size_t grad_ws_bytes; int grad_ws_kind;
    void* grad_ws_lang;
    /* Optional: lsr_fwd_out.lists of the same forward (read only; any number of
     * backwards over that forward may use it). */
    const void* lists;
} lsr_bwd_in;

/* Gradient outputs; NULL = not requested (needs_input_grad False).  Every
 * non-NULL array is fully written (no pre-zeroing needed). */
typedef struct lsr_bwd_out {
    float* dL_dmeans2D;     /* (N,3): [:, :2] = dL/d(NDC xy), [:, 2] = 0 */
    float* dL_dcolors;      /* (N,3): dL/dcolors_precomp */
    float* dL_dlang;        /* (N,D): dL/dlanguage_feature_precomp */
    float* dL_dopacity;     /* (N,1) */
    float* dL_dmeans3D;     /* (N,3) */
    float* dL_dcov3D;       /* (N,6) */
    float* dL_dsh;          /* (N,M,3) */
    float* dL_dscales;      /* (N,3) */
    float* dL_drotations;   /* (N,4) */
    /* Quick (sparse) language input with a gradient: with
     * quick_render set, dL/dlanguage_feature_weights_quick (N,K),
     *   dL/dw[j][m] = sum_p alpha_j(p) T_j(p) dL/dout_lang[idx[j][m]][p];
     * the indices are not differentiable. */
    float* dL_dlang_weights;
    /* Optional hipEvent_t, recorded on `stream` as soon as dL_dlang /
     * dL_dlang_weights are final (before the preprocess backward), so a
     * data-parallel caller can start their all-reduce early (§8e). */
    void* lang_ready_event;
    /* View-factored SH gradient (multi-GPU exchange): when set,
     * (N,3) receives the SH evaluation's colour gradient dL/dRGB of each
     * Gaussian (0 where the SH colour was clamped, 0 for Gaussians outside the
     * view).  dL/dsh of this view is basis(dir) (x) that vector, so a
     * data-parallel caller exchanges these 3 floats (plus the camera centre)
     * instead of the 3*M of dL_dsh and rebuilds the summed SH gradient with
     * lsr_sh_grad_from_views.  dL_dsh may then be NULL. */
    float* dL_drgb_sh;
} lsr_bwd_out;

/* _C.rasterize_gaussians_backward.  With settings.debug set, every stage is
 * synchronised and checked, and inputs / outputs are scanned for NaN/Inf
 * (LSR_ENONFINITE; the offending array is named on stderr). */
int lsr_backward(const lsr_settings* s, const lsr_inputs* in, const lsr_bwd_in* b,
                 lsr_bwd_out* out, lsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* Sum over R views of the SH coefficient gradient, from each view's
 * dL_drgb_sh (lsr_bwd_out): dL_dsh[i][k][c] = sum_r basis_k(dir_ri) *
 * drgb[r][i][c] with dir_ri = normalize(means3D[i] - campos[r]) and the basis
 * of the forward's SH evaluation at `sh_degree` (coefficients above it get 0).
 * Views are summed in order r = 0..R-1, so every rank computes identical
 * values.  means3D (N,3), campos (R,3), drgb (R,N,3), dL_dsh (N,M,3): device
 * pointers; M = max SH coefficients per Gaussian (<= 16). */
int lsr_sh_grad_from_views(int64_t N, int M, int sh_degree, const float* means3D, int R, const float* campos,
                           const float* drgb, float* dL_dsh, void* stream);

/* _C.mark_visible: present[i] = (view-space z of means3D[i]) > 0.2. */
int lsr_mark_visible(int P, const float* means3D, const float* viewmatrix,
                     const float* projmatrix, uint8_t* present, void* stream);

/* Codebook decode of a rendered language weight map;
 * replaces, after render(), the reference's
 *   F = einsum('ldk,lkn->ldn', codebooks.permute(0,2,1), W.view(L, K, H*W))
 *   F = F / (F.norm(dim=1, keepdim=True) + eps)
 * of render_language_feature_map_quick (eval_lerf.py:210-220,
 * backend_renderer.py:16-36); with L = 1 and normalize = 0 it is
 * compute_final_feature_map (scene/gaussian_model.py:545-550).
 * weight_map (L*K, H, W), codebooks (L, K, Df), out (L, Df, H, W), all fp32
 * device pointers.  K must be 64 and Df a multiple of 16. */
int lsr_quick_decode(const float* weight_map, const float* codebooks, int L, int K, int Df, int H, int W,
                     int normalize, float eps, float* out, lsr_alloc_fn alloc, void* alloc_ctx, void* stream);

/* The same decode in two steps for many frames with fixed codebooks (the
 * eval loops of eval_lerf.py decode every view with one model's codebooks):
 * lsr_quick_decode_prepare writes the codebook-only part (fragments, norm
 * factor) into a caller-owned device buffer of lsr_quick_decode_plan_bytes
 * bytes (0 = unsupported shape); lsr_quick_decode_run decodes a frame with it.
 * The plan is valid until the codebooks change.  weight_layout: LSR_LAYOUT_CHW
 * for an (L*K, H, W) weight map, LSR_LAYOUT_HWC for a pixel-major (H, W, L*K)
 * one (lsr_settings.quick_layout); the output is (L, Df, H, W) either way. */
/* The packed code rows (LSR_INDEX_PACKED) of K = 12 code indices per Gaussian:
 * indices (N, 12) of LSR_INDEX_F32 / I32 / I64 index_dtype (fp32 values round
 * half up, u5), packed (N, 4) uint32, 16-B aligned: byte m of row i holds
 * code m + 1 when 0 <= code < quick_dim (0 selects 192), else 0. */
int lsr_quick_pack_codes(const void* indices, int index_dtype, int64_t N, int K, int quick_dim, uint32_t* packed,
                         void* stream);

size_t lsr_quick_decode_plan_bytes(int L, int K, int Df, int normalize);
int lsr_quick_decode_prepare(const float* codebooks, int L, int K, int Df, int normalize, void* plan, void* stream);
int lsr_quick_decode_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int Df, int H,
                         int W, int normalize, float eps, float* out, void* stream);

/* Fused text-query maps of the quick path: what the reference computes from
 * the decoded, normalised (L, H, W, Df) map with
 * OpenCLIPNetwork.get_max_across_quick (eval/openclip_encoder.py:114-139;
 * callers eval_lerf.py:113,160, eval_3d_ovs.py:112,217, demo_prompt.py:122),
 * taken straight from the weight map — the Df-dim map is never written.
 * pos (n_pos, Df) and neg (n_neg, Df) are the text embeddings (fp32 device
 * pointers, used as given: the caller normalises them, as the reference does).
 * lsr_quick_query_prepare writes the (codebooks, query set) part — the
 * projections CB_l E^T (512-term dots in f64) as MFMA fragments and the
 * decode's norm factor — into a caller-owned device buffer of
 * lsr_quick_query_plan_bytes bytes (0 = unsupported shape), valid until the
 * codebooks or the embeddings change.  lsr_quick_query_run writes
 * out (L, n_pos, H, W) fp32 for one frame:
 *   LSR_QUERY_RELEVANCY  min_j softmax(scale * (sim_pos, sim_neg_j))[0]
 *                        = 1 / (1 + exp(scale * (max_j sim_neg_j - sim_pos))),
 *                        scale >= 0 (the reference's is 10), n_neg >= 1;
 *   LSR_QUERY_COSINE     sim_pos = f . e / (|f| + eps) per level (n_neg may be 0).
 * K must be 64, Df a multiple of 16, n_pos >= 1, n_pos + n_neg <= 64 per call
 * (a caller with more positives runs them in chunks); n_pos and n_neg must be
 * the plan's.  Additive to ABI 12. */
enum { LSR_QUERY_RELEVANCY = 0, LSR_QUERY_COSINE = 1 };
size_t lsr_quick_query_plan_bytes(int L, int K, int Df, int n_pos, int n_neg);
int lsr_quick_query_prepare(const float* codebooks, const float* pos, const float* neg, int L, int K, int Df,
                            int n_pos, int n_neg, void* plan, void* stream);
int lsr_quick_query_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int n_pos,
                        int n_neg, int H, int W, int mode, float scale, float eps, float* out, void* stream);

/* Fused open-vocabulary label maps of the quick path: what the reference
 * computes from the decoded, normalised (L, H, W, Df) map with
 * OpenCLIPNetwork.get_semantic_map (eval/openclip_encoder.py:82-94), taken
 * straight from the weight map — the Df-dim map is never written.  labels
 * (n_labels, Df) and neg (n_neg, Df) are the text embeddings (fp32 device
 * pointers, used as given); the columns are the reference's
 * cat([semantic_embeds, neg_embeds]).  Per level and pixel, with
 * s_j = f . e_j / (|f| + eps):
 *   labels_out (L, H, W) int32   argmax_j s_j, the lowest column on exact ties
 *                                (torch.argmax on the CPU), -1 when a negative wins;
 *   scores_out (L, H, W) fp32    1 / sum_j exp(scale (s_j - s_max)), the
 *                                reference's softmax(scale s) at its arg-max;
 *                                optional (NULL: not computed, and the labels
 *                                are the same bits).
 * An all-zero pixel gives label 0 and score 1 / (n_labels + n_neg) exactly.
 * lsr_quick_semantic_prepare writes the (codebooks, label set) part into a
 * caller-owned device buffer of lsr_quick_semantic_plan_bytes bytes
 * (0 = unsupported shape), valid until the codebooks or the embeddings change;
 * n_labels and n_neg of a run must be the plan's.  K must be 64, Df a multiple
 * of 16, n_labels >= 1, n_neg >= 0, n_labels + n_neg <= 256, scale >= 0 (the
 * reference's is 10).
 *
 * lsr_semantic_merge: out (H, W) int32 = per pixel the label of the level
 * with the largest score, the lowest level on ties; level (H, W) uint8 = that
 * level, optional.  The rule is this library's own: the reference returns the
 * per-level maps only.  L <= 255.
 *
 * lsr_semantic_confusion: counts (P, n_classes, n_classes + 1) int64, zeroed
 * by the call; counts[p][g][c] = the pixels with gt (H, W) int32 == g and
 * plane p of pred (P, H, W) int32 == c, column n_classes collecting pred == -1.
 * Pixels with gt outside [0, n_classes) (ignore labels such as 255 or -1) or
 * pred outside [-1, n_classes) are skipped.  n_classes <= 256, P <= 65535,
 * H * W < 2^31.  Integer sums: exact and bit-identical from run to run.
 *
 * LSR_EINVAL: a NULL required pointer, an unknown layout, a negative count or a
 * negative or NaN scale; LSR_EUNSUPPORTED: K != 64, Df % 16 != 0, more than
 * 256 columns or classes, a misaligned pixel-major map, a shape out of range;
 * L, H, W or P = 0: LSR_OK with nothing launched.  Additive to ABI 12. */
size_t lsr_quick_semantic_plan_bytes(int L, int K, int Df, int n_labels, int n_neg);
int lsr_quick_semantic_prepare(const float* codebooks, const float* labels, const float* neg, int L, int K, int Df,
                               int n_labels, int n_neg, void* plan, void* stream);
int lsr_quick_semantic_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int n_labels,
                           int n_neg, int H, int W, float scale, float eps, int32_t* labels_out, float* scores_out,
                           void* stream);
int lsr_semantic_merge(const int32_t* labels, const float* scores, int L, int H, int W, int32_t* out, uint8_t* level,
                       void* stream);
int lsr_semantic_confusion(const int32_t* pred, const int32_t* gt, int P, int H, int W, int n_classes, int64_t* counts,
                           void* stream);

/* Post-process of the relevancy maps (eval_lerf.py:104-200; eval_3d_ovs.py:
 * 102-107, 215-260) on planes = L * n_prompt independent (H, W) fp32 planes
 * (level-major: plane = l * n_prompt + q), in two passes with caller-owned
 * outputs and a caller-owned workspace of lsr_query_post_workspace_bytes bytes
 * (0 = unsupported shape: more than 65535 planes or 32-row tile rows, or
 * H * W >= 2^31).  Nothing is synchronised, every result is bit-identical from
 * run to run, and rel is never written.
 *
 * lsr_query_smooth: avg = AvgPool2d(kernel, stride 1, padding (kernel - 1) / 2,
 * count_include_pad=False)(rel) as row sums then column sums of at most
 * `kernel` terms each, divided by the in-image tap count; blend =
 * 0.5 (avg + rel).  avg and blend are optional (NULL: not written).  Per plane
 * stats (planes, 3) = {min blend, max blend, max avg} and loc (planes, 2) =
 * {row-major index of the first pixel attaining max avg, number of pixels
 * attaining it}.  kernel odd, 1..63.
 *
 * lsr_query_mask: o = clip(2 ((blend - min) / (max - min + 1e-9f)) - 1, 0, 1)
 * with min, max from stats; raw = o > thresh; mask (planes, H, W) uint8 = 1
 * where more than half of the in-image pixels of the smooth_kernel^2 window are
 * set in raw (integer arithmetic; smooth_kernel odd, 1..15).  counts
 * (planes, 3) = {set pixels, intersection, union} with the annotation mask
 * gt_masks (n_prompt, H, W) uint8 (non-zero = inside) of the plane's prompt
 * (NULL: intersection and union are 0); masked_sum (planes) = sum of blend over
 * the mask.
 *
 * LSR_EINVAL: an even or non-positive kernel, a NULL required pointer, planes
 * not a multiple of n_prompt; LSR_EUNSUPPORTED: kernel size or shape out of
 * range; planes, H or W = 0: LSR_OK with nothing launched.  Additive to ABI 12. */
size_t lsr_query_post_workspace_bytes(int planes, int H, int W);
int lsr_query_smooth(const float* rel, int planes, int H, int W, int kernel, float* avg, float* blend, float* stats,
                     int64_t* loc, void* workspace, void* stream);
int lsr_query_mask(const float* blend, const float* stats, const uint8_t* gt_masks, int planes, int n_prompt, int H,
                   int W, float thresh, int smooth_kernel, uint8_t* mask, int64_t* counts, float* masked_sum,
                   void* workspace, void* stream);

/* The viewers' query maps, one (n_pos, H, W) fp32 map per prompt taken from
 * all levels of a pixel at once — the decoded (L, Df, H, W) map is never
 * written (backend_renderer.py:193-233, demo_prompt.py:118-150).  With
 * f_l = F_l / (|F_l| + eps) the normalised decode of level l:
 *   LSR_HEAT_SUMMED_COSINE   s = sum_l f_l, out[q] = s . pos_q / (|s| + eps)
 *                            (the render server; negatives are ignored);
 *   LSR_HEAT_MEAN_RELEVANCY  (sum_l rel_l[q]) / L in level order, rel_l the
 *                            relevancy of lsr_quick_query_run (the prompt demo;
 *                            scale >= 0, n_neg >= 1).
 * An all-zero pixel gives exactly 0 / 0.5.  lsr_quick_heat_prepare writes the
 * (codebooks, query set) part — the query plan's projections and norm factors
 * and the f64 Cholesky factor of the stacked (L K) x (L K) Gram matrix, from
 * which |s| is a sum of squares — into a caller-owned device buffer of
 * lsr_quick_heat_plan_bytes bytes (0 = unsupported shape), valid until the
 * codebooks or the embeddings change; it is not a query plan.  K must be 64,
 * Df a multiple of 16, L <= 3, n_pos >= 1, n_pos + n_neg <= 64; n_pos and
 * n_neg must be the plan's.
 *
 * lsr_heat_frame: colour, blend and pack.  maps (planes, H, W) fp32, stats
 * (planes, 3) fp32 = {min, max, unused} per plane (the rows lsr_query_smooth
 * writes; with kernel = 1 and NULL avg / blend they are the maps' exact
 * minimum and maximum), rgb (3, H, W) fp32 or NULL, lut (256, 3) uint8 ->
 * out (planes, H, W, 3) uint8, RGB, pixel-major.  Per plane, every operation
 * in fp32 and rounded on its own:
 *   gate   max < threshold or (max - min) < min_range: v = 0 on the plane
 *   LSR_CURVE_UPPER_HALF  t = (x - min) / ((max - min) + 1e-9f), v = clip(t * 2 - 1, 0, 1)
 *   LSR_CURVE_POWER4      t = (x - min) / ((max - min) + 1e-8f), v = (t * t) * (t * t)
 *   heat   = lut[(int)(v * 255.f) clamped to 0..255]
 *   out_c  = heat_c, or with rgb (uint8)(clip(rgb_c * (1.f - alpha) + ((float)heat_c / 255.f) * alpha, 0, 1) * 255.f)
 * Non-finite inputs give unspecified bytes (the table is still indexed inside
 * 0..255).  Bit-identical from run to run.
 *
 * LSR_EINVAL: a NULL required pointer, an unknown layout, mode or curve, a
 * negative or NaN scale or alpha, alpha > 1, n_pos < 1; LSR_EUNSUPPORTED: a
 * shape out of range (K, L > 3, n_pos + n_neg > 64, mean relevancy without
 * negatives, a misaligned pixel-major map, more than 65535 planes, H * W near
 * 2^31); L, H, W or planes = 0: LSR_OK with nothing launched.  Additive to ABI 12. */
enum { LSR_HEAT_SUMMED_COSINE = 0, LSR_HEAT_MEAN_RELEVANCY = 1 };
enum { LSR_CURVE_UPPER_HALF = 0, LSR_CURVE_POWER4 = 1 };
size_t lsr_quick_heat_plan_bytes(int L, int K, int Df, int n_pos, int n_neg);
int lsr_quick_heat_prepare(const float* codebooks, const float* pos, const float* neg, int L, int K, int Df,
                           int n_pos, int n_neg, void* plan, void* stream);
int lsr_quick_heat_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int n_pos, int n_neg,
                       int H, int W, int mode, float scale, float eps, float* out, void* stream);
int lsr_heat_frame(const float* maps, const float* stats, const float* rgb, const uint8_t* lut, int planes, int H, int W,
                   int curve, float threshold, float min_range, float alpha, uint8_t* out, void* stream);

/* Fused top-k soft codes (replaces softmax_to_topk_soft_code,
 * utils/vq_utils.py:9-24; get_weights_and_indices, :26-40; the per-level
 * loop of GaussianModel.get_render_weights, scene/gaussian_model.py:510-518;
 * and the level-offset concatenation of eval_lerf.py:340-348).
 * logits (N, L*K) fp32: L levels of K-way codes; K in {64,128,192,256},
 * 1 <= k <= K.  Outputs (any may be NULL, at least one not):
 *   dense      (N, L*K) fp32: y*mask / (sum(y*mask) + 1e-10) per level;
 *   sparse_w   (N, L*k) fp32: the k non-zeros of each level in ascending
 *              channel order;
 *   sparse_idx (N, L*k) of LSR_INDEX_* idx_dtype: their channel indices,
 *              + l*K for level l when level_offset != 0.
 * Top-k ties go to the lower channel (torch.topk's tie order is
 * implementation-defined). */
int lsr_topk_code_forward(const float* logits, int64_t N, int L, int K, int k, float* dense, float* sparse_w,
                          void* sparse_idx, int idx_dtype, int level_offset, void* stream);
/* dL/dlogits (N, L*K) from dL/ddense (N, L*K): the autograd chain of
 * softmax_to_topk_soft_code (mask recomputed from the logits). */
int lsr_topk_code_backward(const float* logits, const float* grad_dense, int64_t N, int L, int K, int k,
                           float* grad_logits, void* stream);
/* dL/dlogits (N, L*K) from dL/dsparse_w (N, L*k): the gradient of the packed
 * weights (ascending channel order, as lsr_topk_code_forward's sparse_w),
 * e.g. lsr_bwd_out.dL_dlang_weights of a quick-mode render; the dense code
 * gradient is never formed (the sparse training path). */
int lsr_topk_code_backward_sparse(const float* logits, const float* grad_weights, int64_t N, int L, int K, int k,
                                  float* grad_logits, void* stream);

/* Language-feature cosine loss of the feature-mode training step (SURVEY
 * §8f rank 4; train.py:151-164 with vq_layer_num = 1, layer_idx = 0):
 *   f[:, p]  = codebooks[0]^T w_p        compute_layer_feature_map,
 *                                        scene/gaussian_model.py:533-543
 *   gt[:, p] = features[seg[p]], mask[p] = seg[p] != -1
 *                                        get_language_feature, scene/cameras.py:59-96
 *   loss     = 1 - mean_p cos(f_p*mask_p, gt_p*mask_p)   cos_loss,
 *                                        utils/loss_utils.py:24-25 (eps 1e-8)
 * weight_map (K, H, W), codebooks (K, Df), features (S, Df) fp32; seg (H, W)
 * int32 segment ids, -1 (or any id outside [0, S)) = masked.  K must be 64,
 * Df a multiple of 16.  Nothing of size Df x pixels is materialised
 * (everything factors through the K-dim code space).  Forward writes loss[0]
 * and/or pixel_stats (2, H, W) (|f_p| and f_p.gt_p; either may be NULL).
 * Backward writes grad_weight_map (K, H, W) and grad_codebooks (K, Df), both
 * scaled by the device scalar *grad_loss, from the forward's pixel_stats
 * (NULL: recomputed).  Workspace via alloc (LSR_BUF_LOSS). */
int lsr_lang_loss_forward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                          const int32_t* seg, const float* features, int S, float* loss, float* pixel_stats,
                          lsr_alloc_fn alloc, void* alloc_ctx, void* stream);
int lsr_lang_loss_backward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                           const int32_t* seg, const float* features, int S, const float* pixel_stats,
                           const float* grad_loss, float* grad_weight_map, float* grad_codebooks, lsr_alloc_fn alloc,
                           void* alloc_ctx, void* stream);

/* L1 loss of the same step (train.py:157-167 with --l1_loss; normalize != 0
 * is --normalize), same tensors, limits and masking rule as the cosine pair:
 *   u_p  = f_p, or f_p / (|f_p| + 1e-10) with normalize
 *   loss = mean over all Df*H*W elements of mask_p |u_pd - gt_pd|
 *                                        l1_loss, utils/loss_utils.py:18-19
 * Nothing of size Df x pixels is materialised: f is formed 16 features x 64
 * pixels at a time on the exact-f32 matrix units and compared in registers.
 * The loss is summed in a fixed order (bit-identical from run to run).
 * Forward writes loss[0] and, with normalize, pixel_stats (2, H, W) (|f_p|
 * and sum_d u_pd sign(u_pd - gt_pd)); either may be NULL, and without
 * normalize pixel_stats is neither written nor read.  Backward writes
 * grad_weight_map (K, H, W) and grad_codebooks (K, Df), both scaled by the
 * device scalar *grad_loss, with sign(0) = 0 and the norm's zero subgradient
 * at |f_p| = 0, from the forward's pixel_stats (NULL: recomputed).
 * Workspace via alloc (LSR_BUF_LOSS). */
int lsr_lang_l1_forward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                        const int32_t* seg, const float* features, int S, int normalize, float* loss,
                        float* pixel_stats, lsr_alloc_fn alloc, void* alloc_ctx, void* stream);
int lsr_lang_l1_backward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                         const int32_t* seg, const float* features, int S, int normalize, const float* pixel_stats,
                         const float* grad_loss, float* grad_weight_map, float* grad_codebooks, lsr_alloc_fn alloc,
                         void* alloc_ctx, void* stream);

/* Photometric loss of the RGB training step (train.py:170-173,
 * utils/loss_utils.py:18-71): image and gt are planes = B*C contiguous fp32
 * planes of H x W.  Forward writes out[0] = mean |image - gt| and out[1] = mean
 * SSIM (11-tap Gaussian window, sigma 1.5, zero padding of 5, C1 = 1e-4,
 * C2 = 9e-4), both over planes*H*W and bit-identical from run to run, and, when
 * partials is given, the per-pixel derivative maps (3, planes, H, W) the
 * backward gathers from.  Backward writes
 *   grad_image = grad_out[0] d out[0]/d image + grad_out[1] d out[1]/d image
 * (sign(0) = 0) with grad_out a device float[2]; nothing flows to gt.
 * The caller's loss is (1 - lambda) out[0] + lambda (1 - out[1]).
 *
 * LSR_EINVAL: planes, H or W < 1, a NULL image, gt, out or alloc (forward), a
 * NULL partials, grad_out or grad_image (backward); LSR_EUNSUPPORTED:
 * planes*H*W >= 2^31; LSR_ENOMEM: alloc returned NULL.  Workspace via alloc
 * (LSR_BUF_LOSS).  Additive to ABI 12. */
int lsr_photo_loss_forward(const float* image, const float* gt, int planes, int H, int W,
                           float* out /* [2]: mean |x-y|, mean SSIM */, float* partials /* (3, planes, H, W) or NULL */,
                           lsr_alloc_fn alloc, void* alloc_ctx, void* stream);
int lsr_photo_loss_backward(const float* image, const float* gt, int planes, int H, int W,
                            const float* partials, const float* grad_out /* device float[2] */,
                            float* grad_image, void* stream);

/* k-means codebook initialisation of the feature phase: Lloyd's iteration over
 * the (M, D) fp32 table of 2-D language features, per level what
 * ResidualVectorQuantizationWithClustering.fit_quantizers (utils/vq_utils.py:43-104,
 * train.py:78-85) does on the host with sklearn and an M x K torch.cdist.
 *
 * lsr_kmeans_prepare lays the (K, D) centres out for the search in workspace
 * (lsr_kmeans_workspace_bytes(M, K, D) bytes, device, 256-B aligned; the part it
 * writes does not depend on M).  lsr_kmeans_assign then gives per row the
 * nearest prepared centre by score_k = |c_k|^2 - 2 x.c_k (exact-f32 MFMA, ties
 * to the lowest index, as numpy / torch argmin on CPU): assign (M) int32, dist
 * (M) = max(score + |x|^2, 0), and optionally residual_out (M, D) = x -
 * c[assign] (must not alias x).  lsr_kmeans_update forms centers_out (K, D) =
 * the mean of each cluster's rows and counts_out (K) int32 from x and assign
 * (an index outside [0, K) is skipped); a cluster without rows keeps its
 * prepared centre and reports 0.  It then prepares centers_out in workspace,
 * so assign / update alternate with no further call.  No float atomics and a
 * split that depends on (M, K, D) only: bit-identical from run to run.
 *
 * LSR_EINVAL: K outside 1..256, D outside 4..1024 or not a multiple of 4, M < 0
 * or M >= 2^31, a NULL or not 16-B aligned x, centers, workspace or
 * centers_out, a residual_out that is not 16-B aligned or equals x, a NULL
 * assign, dist or counts_out.  M = 0 is a no-op
 * (nothing is read or written).  lsr_kmeans_workspace_bytes returns 0 for a
 * shape that is not taken.  Additive to ABI 12. */
size_t lsr_kmeans_workspace_bytes(int64_t M, int K, int D);
int lsr_kmeans_prepare(const float* centers, int K, int D, void* workspace, void* stream);
int lsr_kmeans_assign(const float* x, int64_t M, int D, int K, const void* workspace, int32_t* assign, float* dist,
                      float* residual_out /* (M, D) or NULL */, void* stream);
int lsr_kmeans_update(const float* x, const int32_t* assign, int64_t M, int D, int K, void* workspace,
                      float* centers_out, int32_t* counts_out, void* stream);

/* SAM mask NMS and segment maps of the preprocess step that writes
 * <image>_s.npy: mask_nms (preprocess.py:215-279) and mask2segmap with create's
 * level offsets (preprocess.py:304-317, :145-157), on bit-packed masks.
 *
 * lsr_mask_pack packs (N, H, W) bytes (nonzero = set) into words (N, W64),
 * W64 = ceil(H W / 64): bit b of word w is pixel 64 w + b in row-major order,
 * bits past H W are zero; area (N) is each mask's popcount.
 * lsr_mask_pair_counts fills inter (N, N): inter[i][j] = |mask order[i] AND
 * mask order[j]| for i <= j (order NULL: the identity), 0 below the diagonal.
 * Integer accumulation only: exact and identical from run to run.
 * lsr_mask_nms_select does the pair counts into workspace
 * (lsr_mask_nms_workspace_bytes(N) bytes, device, 16-B aligned; it starts with
 * the (N, N) int32 table) and then, in one launch with no host read-back,
 * decides: order (N) is the rank order (scores descending, stable), conf (N)
 * is per rank score > score_thr.  With I = inter[i][j], A = area, all fp32:
 *   iou = f(I) / f(A_i + A_j - I),  a = f(I) / f(A_i),  b = f(I) / f(A_j),
 *   U[i][j] = 1 - b a if a < 0.5 and b >= 0.85,  L[j][i] = 1 - b a if a >= 0.85 and b < 0.5,
 *   iou_max[c] = max(0, max_{i<c} iou[i][c]),  u_max[c] = max(0, max_{i<c} U[i][c]),
 *   l_max[c] = max(0, max_{r>c} L[r][c], U[c-1][c])   (the reference's tril(diagonal=1)),
 *   keep[c] = iou_max[c] <= (float)iou_thr and conf[c] and u_max[c] <= cut and l_max[c] <= cut,
 *   cut = (float)(1.0 - inner_thr);
 * the maxima propagate NaN (an empty pair's 0 / 0 drops its column); a
 * criterion among conf, inner-u, inner-l that no rank passes is set for ranks
 * 0 .. min(3, N) - 1 instead.  keep (N) is per rank, criteria (N, or NULL) the
 * LSR_MASK_CRIT_* bits per rank after the fallbacks, selected (N int64, the
 * first *count valid) the kept input indices in rank order.  An order entry
 * outside [0, N) reads as an empty mask.
 * lsr_mask_segmaps writes out (4, H, W), fp32 (LSR_INDEX_F32) or int32
 * (LSR_INDEX_I32): per level l the highest k < counts[l] whose mask kept[l][k]
 * (of the masks[l] packed masks words[l]) covers the pixel, plus offsets[l];
 * -1 where none does.  The four arrays are host arrays of 4; a level with
 * counts[l] = 0 may have NULL pointers.
 *
 * LSR_EUNSUPPORTED: N (masks[l], counts[l]) > LSR_MASK_MAX_N, H W >
 * LSR_MASK_MAX_PIXELS (every count must be exact in fp32).  LSR_EINVAL: N < 0,
 * H or W < 1, a NULL or misaligned (words: 8 B, workspace: 16 B) pointer, a
 * negative count or offset, an index_type other than the two.  N = 0 (pack,
 * pair counts, select): LSR_OK, nothing is read or written.  All checks come
 * before any device call.  lsr_mask_nms_workspace_bytes returns 0 for an N that
 * is not taken.  Additive to ABI 12. */
#define LSR_MASK_MAX_N 4096
#define LSR_MASK_MAX_PIXELS (1 << 24)
#define LSR_MASK_PAIR_TILE 64   /* masks per side of a pair-count tile */
#define LSR_MASK_WORD_CHUNK 32  /* 64-bit words of each mask a pair-count step stages */
#define LSR_MASK_CRIT_IOU 1
#define LSR_MASK_CRIT_CONF 2
#define LSR_MASK_CRIT_INNER_U 4
#define LSR_MASK_CRIT_INNER_L 8
size_t lsr_mask_nms_workspace_bytes(int N);
int lsr_mask_pack(const uint8_t* masks, int N, int H, int W, uint64_t* words, int32_t* area, void* stream);
int lsr_mask_pair_counts(const uint64_t* words, int N, int H, int W, const int32_t* order /* or NULL */,
                         int32_t* inter, void* stream);
int lsr_mask_nms_select(const uint64_t* words, const int32_t* area, int N, int H, int W, const int32_t* order,
                        const uint8_t* conf, double iou_thr, double inner_thr, void* workspace, uint8_t* keep,
                        uint8_t* criteria /* or NULL */, int64_t* selected, int32_t* count, void* stream);
int lsr_mask_segmaps(const uint64_t* const* words, const int32_t* const* kept, const int32_t* masks,
                     const int32_t* counts, const int32_t* offsets, int H, int W, int index_type, void* out,
                     void* stream);

/* The CLIP input tiles of the kept masks: mask2segmap's get_seg_img, pad_img and
 * cv2.resize per mask (preprocess.py:304-317, :191-206), the / 255 of :315 and
 * encode_image's normalisation and cast (:105-107), from the packed masks.
 *
 * lsr_mask_boxes writes boxes (N, 4) int32 x, y, w, h: the tight extents of each
 * packed mask (w = xmax - x + 1, h = ymax - y + 1; an empty mask: 0, 0, 0, 0).
 * lsr_clip_tiles writes n tiles of S x S pixels; tile t is mask keep[t] (keep
 * NULL: mask t, and n <= N).  image is (H, W, 3) uint8, boxes (N, 4) int32 is
 * indexed by mask.  Per tile, all in integers (DESIGN "CLIP tiles"):
 *   crop   x0 = clamp(x, 0, W), x1 = clamp(x + w, 0, W), cw = max(x1 - x0, 0), likewise y0, ch;
 *   pad    to a square of side l = max(cw, ch), the crop centred along its shorter side
 *          (offset |ch - cw| / 2, rounded down); a pixel outside the crop or with its mask
 *          bit clear is (0, 0, 0);
 *   resize l x l -> S x S as OpenCV's 8-bit INTER_LINEAR: source coordinate
 *          f = (float)((d + 0.5) * (1.0 / ((double)S / l)) - 0.5), 11-bit coefficients
 *          rint(f * 2048), out = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2.
 * A tile with l = 0, or with a keep entry outside [0, N), is all zeros.
 * out_type LSR_TILE_U8: out (n, S, S, 3) uint8, lut unused.  LSR_TILE_UNIT: out
 * (n, 3, S, S) fp32 = lut[c][v], lut (3, 256) fp32.  LSR_TILE_CLIP: out
 * (n, 3, S, S) fp16 = lut[c][v], lut (3, 256) fp16.  The caller fills lut (v / 255
 * and its normalised form); the kernel does no float arithmetic on pixels.
 *
 * LSR_EINVAL, before any device call: N or n outside 0 .. LSR_MASK_MAX_N, H or
 * W < 1 or H W > LSR_MASK_MAX_PIXELS, S outside 1 .. LSR_TILE_MAX_SIDE, an unknown
 * out_type, keep NULL with n > N, a NULL or misaligned (words: 8 B; boxes, keep:
 * 4 B; lut, fp32 / fp16 out: their element) pointer, lut NULL for a float form.
 * N = 0 (boxes) and n = 0 (tiles): LSR_OK, nothing is read or written.  Additive
 * to ABI 12. */
#define LSR_TILE_MAX_SIDE 1024
#define LSR_TILE_U8 0
#define LSR_TILE_UNIT 1
#define LSR_TILE_CLIP 2
int lsr_mask_boxes(const uint64_t* words, int N, int H, int W, int32_t* boxes, void* stream);
int lsr_clip_tiles(const uint8_t* image, int H, int W, const uint64_t* words, int N,
                   const int32_t* keep /* or NULL */, const int32_t* boxes, int n, int S,
                   const void* lut /* NULL for LSR_TILE_U8 */, int out_type, void* out, void* stream);

/* Fused Adam step: the update of torch.optim.Adam as the
 * reference builds it (scene/gaussian_model.py:234-255, no amsgrad), one pass
 * over n fp32 elements of params / grads / exp_avg / exp_avg_sq (device
 * pointers, same layout).  step is the 1-based step count after increment;
 * the scalars are doubles (Python floats) and the bias corrections are
 * formed in double on the host, as torch does. */
int lsr_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int64_t step, void* stream);

/* GaussianModel.densify_and_prune of the RGB phase (scene/gaussian_model.py:352-504,
 * every 100 iterations, train.py:246-258) as one gather over the six parameter
 * groups and their Adam moments.  Groups, in this order, all fp32 row-major with
 * N rows: xyz (3), f_dc (3), f_rest (rest_width = 3 (coeffs - 1)), opacity (1),
 * scaling (3, log-scales), rotation (4, raw quaternion).
 *
 * Per row i: g = accum / denom with NaN -> 0 (x / 0 = inf stays and is selected),
 * ms = max_j exp(scaling_j); clone: |g| >= max_grad and ms <= dense_thresh;
 * split: g >= max_grad and ms > dense_thresh.  A split row is replaced by two
 * children r = 0, 1: xyz' = build_rotation(rotation) (exp(scaling) * noise[i][r]) + xyz,
 * scaling' = log(exp(scaling) / 1.6), the rest copied.  Every surviving row
 * (originals, clones, children with scaling') is dropped when
 * sigmoid(opacity) < min_opacity, or, with prune_big != 0, when its
 * max_j exp(scaling_j) > big_thresh.  (The reference zeroes max_radii2D before
 * its final prune, so its screen-size term never fires; it is not an input.)
 * Output rows, each segment in input order: kept originals, kept clones, kept
 * round-0 children, kept round-1 children.  Moments are copied for the first
 * segment and zero elsewhere.  No atomics: bit-reproducible.
 *
 * lsr_densify_plan classifies, scans and fills the row map in workspace
 * (lsr_densify_workspace_bytes(N) bytes, device, 256-B aligned) and returns in
 * the host array counts[LSR_DENSIFY_COUNTS] = {the four segment sizes, rows
 * selected for cloning, rows selected for splitting} after synchronising the
 * stream (the one host read-back, like lsr_fwd_out.num_rendered).  The caller
 * sizes the outputs to n_out = counts[0] + .. + counts[3] rows and calls
 * lsr_densify_apply with the same N and workspace: one launch writes every
 * non-NULL dst tensor (a NULL dst skips that tensor, e.g. moments of an
 * optimiser without state; its src is then ignored).  noise is (N, 2, 3)
 * standard-normal samples indexed by parent row and round.
 *
 * LSR_EINVAL: N < 0, rest_width < 0, max_grad <= 0 or NaN (clones must never be
 * split again), a NULL required pointer, n_out < 0; LSR_EUNSUPPORTED: N > 2^28;
 * N == 0 (plan: counts all 0) and n_out == 0 (apply) are no-ops.  Additive to ABI 12. */
#define LSR_DENSIFY_GROUPS 6
#define LSR_DENSIFY_XYZ 0
#define LSR_DENSIFY_F_DC 1
#define LSR_DENSIFY_F_REST 2
#define LSR_DENSIFY_OPACITY 3
#define LSR_DENSIFY_SCALING 4
#define LSR_DENSIFY_ROTATION 5
#define LSR_DENSIFY_COUNTS 6
#define LSR_DENSIFY_MAX_ROWS (1LL << 28)
size_t lsr_densify_workspace_bytes(int64_t N);
int lsr_densify_plan(int64_t N, const float* accum, const float* denom, const float* scaling, const float* opacity,
                     float max_grad, float dense_thresh, float min_opacity, int prune_big, float big_thresh,
                     void* workspace, int64_t* counts /* host [LSR_DENSIFY_COUNTS] */, void* stream);
int lsr_densify_apply(int64_t N, int64_t n_out, const void* workspace, int rest_width,
                      const float* const* src /* [3][LSR_DENSIFY_GROUPS]: parameter, exp_avg, exp_avg_sq */,
                      float* const* dst /* same layout; NULL entries skipped */, const float* noise, void* stream);
/* GaussianModel.reset_opacity (scene/gaussian_model.py:303-306), in place over n
 * elements: opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)), exp_avg and
 * exp_avg_sq (either may be NULL) zeroed. */
int lsr_reset_opacity(int64_t n, float* opacity, float* exp_avg, float* exp_avg_sq, void* stream);

/* simple_knn._C.distCUDA2 (scene/gaussian_model.py:20,194): for points
 * (N, 3) fp32, out[i] = mean of the three smallest squared distances
 * dx*dx + dy*dy + dz*dz to points j != i (exact; FLT_MAX for missing
 * neighbours when N < 4).  Workspace (~40 B/point) via alloc. */
int lsr_knn_dist2(const float* points, int64_t N, float* out, lsr_alloc_fn alloc, void* alloc_ctx, void* stream);

const char* lsr_strerror(int code);
int lsr_abi_version(void);

/* Process-wide options.  LSR_OPT_BIN_MODE picks the forward's tile binning:
 * LSR_BIN_SORTED_TILES (= LSR_BIN_AUTO, the default) scatters (depth, id) keys
 * into the tile buckets and sorts each bucket.  (ABI <= 8's LSR_BIN_ORDERED, a
 * depth-ordered mode measured slower at every size, is no longer built: the
 * value is rejected with LSR_EINVAL.)  LSR_OPT_LISTS_MAX_MB (default 2048): a
 * forward with a backward pending writes the backward's per-block candidate
 * lists (128 B per tile instance) only while they fit this many MiB; above it
 * the backward re-stages from the tile lists (identical results).  LSR_EINVAL
 * for an unknown option/value. */
#define LSR_OPT_BIN_MODE 1
#define LSR_OPT_LISTS_MAX_MB 2
/* LSR_OPT_SPLIT_PREPROCESS (default 1): a forward with SH colours of at least
 * 2^19 Gaussians evaluates the SH colour on a library-owned second stream
 * of the current device, concurrent with the tile binning (the geometry the
 * binning needs stays on the caller's stream, and the render waits for both);
 * 0: one fused preprocess kernel on the caller's stream.  Results identical. */
#define LSR_OPT_SPLIT_PREPROCESS 3
/* LSR_OPT_DETERMINISTIC (default 0): 1 makes lsr_backward bit-reproducible.
 * The render backward's cross-block sums (every per-Gaussian gradient is a sum
 * of per-8x8-block partials, added by atomics in whatever order the blocks
 * finish) are accumulated as 64-bit fixed-point integers, whose addition is
 * associative: one binary exponent per (Gaussian, gradient column) chosen from
 * an a-priori bound (the launch's max |dL/dout| and max |feature|, the
 * Gaussian's radius, the image size), so the sum cannot overflow, and each
 * block partial is rounded once to 2^-s (s is 30-60 bits below the bound).
 * Two backwards of the same inputs give identical bits.  A non-finite input or
 * term turns every gradient of that call into NaN (never a silently wrong
 * value).  Costs one bound pass, a zeroed 8-B-per-value accumulator, 64-bit
 * atomics (twice the atomic bytes) and one conversion pass. */
#define LSR_OPT_DETERMINISTIC 4
#define LSR_BIN_AUTO 0
#define LSR_BIN_SORTED_TILES 1
#define LSR_BIN_ORDERED 2
int lsr_set_option(int option, int64_t value);
int lsr_get_option(int option, int64_t* value);

/* A non-blocking HIP stream on the current device (no implicit
 * synchronisation with the legacy default stream), created with the HIP
 * runtime this library uses; for callers that overlap renders across streams
 * (langsplatv2_amd.view_stream).  lsr_stream_destroy releases it. */
int lsr_stream_create(void** stream);
int lsr_stream_destroy(void* stream);

/* Dense language channel sets compiled into this build (ascending; D is
 * rounded up to the next set).  Returns the largest supported D. */
int lsr_max_lang_dim(void);

/* Diagnostics: per-stage HIP-event timing on the caller's stream (used by
 * bench.py for the live roofline).  One process-wide, thread-safe timer
 * (atomic switch, mutex-guarded event pool; autograd runs the backward on its
 * own thread): off by default, and while off the entry points above read one
 * atomic flag per stage and nothing else.
 * lsr_profile_query fills up to max_stages (name, total ms, call count)
 * triples since the last reset and returns the number filled. */
void lsr_profile_enable(int on);
/* Restrict the timed stages to a comma-separated list of stage names
 * ("render_bwd,render_fwd"); NULL or "" selects every stage.  Each timed
 * stage adds two event records (a few us of stream idle each), so bench.py
 * times only the roofline kernel inside its timed region.  Returns
 * LSR_EINVAL for an unknown name (mask unchanged). */
int lsr_profile_stages(const char* names);
void lsr_profile_reset(void);
int lsr_profile_query(const char** names, double* ms, int64_t* calls, int max_stages);

#ifdef __cplusplus
}
#endif
#endif
