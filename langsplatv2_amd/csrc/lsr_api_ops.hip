// lsr_api_ops.hip — the C ABI's stateless entry points: each validates its
// arguments, requests a workspace where it needs one and enqueues one kernel
// family on the caller's stream.  The codes, and which of two failing checks
// wins, are behaviour: tools/asan_host_check.py holds the table.
#include <math.h>
#include "lsr_api_common.h"

using namespace lsr;

namespace {

// the decode / query kernels' codebooks: L levels of K = 64 codes, Df a multiple of 16
int codebook_args(int L, int K, int Df)
{
    if (L < 0 || Df <= 0 || (Df % 16) != 0) return LSR_EINVAL;
    return K == 64 ? LSR_OK : LSR_EUNSUPPORTED;
}

bool layout_ok(int layout) { return layout == LSR_LAYOUT_CHW || layout == LSR_LAYOUT_HWC; }

bool misaligned16(const void* p) { return ((uintptr_t)p % 16) != 0; }

int lang_loss_args(const float* wm, const float* cb, int K, int Df, int H, int W, const int32_t* seg,
                   const float* feat, int S)
{
    if (K <= 0 || Df <= 0 || H <= 0 || W <= 0 || S < 0) return LSR_EINVAL;
    if (K != 64 || (Df % 16) != 0) return LSR_EUNSUPPORTED;
    if (!wm || !cb || !seg || (S > 0 && !feat)) return LSR_EINVAL;
    return LSR_OK;
}

int photo_loss_args(const float* image, const float* gt, int planes, int H, int W)
{
    if (planes < 1 || H < 1 || W < 1 || !image || !gt) return LSR_EINVAL;
    const int64_t rows = (int64_t)planes * H;   // 32-bit element offsets: planes H W < 2^31
    return rows > 0x7fffffffLL || rows * W > 0x7fffffffLL ? LSR_EUNSUPPORTED : LSR_OK;
}

// utils/loss_utils.py:31-33 gaussian(11, 1.5), bit for bit: exp per tap in double, held in
// an fp32 tensor, so the sum (torch's: the correctly rounded one) and the division are fp32
PhotoTaps photo_taps()
{
    PhotoTaps t;
    double sum = 0.0;
    for (int i = 0; i < 11; i++) sum += t.w[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    const float fsum = (float)sum;
    for (int i = 0; i < 11; i++) t.w[i] = t.w[i] / fsum;
    return t;
}

// every shape the k-means kernels do not take is an invalid argument
int kmeans_args(int64_t M, int K, int D)
{
    return M < 0 || M > 0x7fffffffLL || K < 1 || K > 256 || D < 4 || D > 1024 || (D % 4) != 0 ? LSR_EINVAL : LSR_OK;
}

// a mask count or frame beyond what the mask kernels are built for is unsupported, anything else invalid
int mask_args(int N, int H, int W)
{
    if (N < 0 || H < 1 || W < 1) return LSR_EINVAL;
    return N > LSR_MASK_MAX_N || (int64_t)H * W > LSR_MASK_MAX_PIXELS ? LSR_EUNSUPPORTED : LSR_OK;
}

bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// the tile entry points take the mask kernels' limits and call everything beyond them invalid
int tile_args(int N, int n, int H, int W, int S)
{
    if (N < 0 || N > LSR_MASK_MAX_N || n < 0 || n > LSR_MASK_MAX_N || H < 1 || W < 1 ||
        (int64_t)H * W > LSR_MASK_MAX_PIXELS || S < 1 || S > LSR_TILE_MAX_SIDE)
        return LSR_EINVAL;
    return LSR_OK;
}

// a code count the kernels are not built for is unsupported, anything else invalid
int topk_code_args(int64_t N, int L, int K, int k)
{
    if (N >= 0 && L >= 1 && K >= 64 && K <= 256 && (K % 64) == 0 && k >= 1 && k <= K &&
        N <= (int64_t)0x7fffffff / ((int64_t)L * K))
        return LSR_OK;
    return (K % 64 || K > 256) && K > 0 ? LSR_EUNSUPPORTED : LSR_EINVAL;
}

// dense: g is dL/d(dense codes); sparse: dL/dweights of the packed (N, L*k) form
int topk_code_backward(const float* logits, const float* g, int64_t N, int L, int K, int k, float* grad_logits,
                       void* stream, bool sparse)
{
    LSR_TRY(topk_code_args(N, L, K, k));
    if (N == 0) return LSR_OK;
    if (!logits || !g || !grad_logits) return LSR_EINVAL;
    LSR_HIP(launch_topk_code_bwd(logits, g, N, L, K, k, grad_logits, (hipStream_t)stream, sparse));
    return LSR_OK;
}

}  // namespace

extern "C" {

int lsr_quick_decode(const float* weight_map, const float* codebooks, int L, int K, int Df, int H, int W,
                     int normalize, float eps, float* out, lsr_alloc_fn alloc, void* alloc_ctx, void* stream)
{
    if (H < 0 || W < 0) return LSR_EINVAL;
    LSR_TRY(codebook_args(L, K, Df));
    if (L == 0 || H == 0 || W == 0) return LSR_OK;
    if (!weight_map || !codebooks || !out) return LSR_EINVAL;
    void* ws = nullptr;
    const size_t wsb = quick_decode_workspace_bytes(L, K, Df, normalize);
    if (wsb) {
        if (!alloc) return LSR_EINVAL;
        ws = alloc(alloc_ctx, wsb, LSR_BUF_DECODE);
        if (!ws) return LSR_ENOMEM;
    }
    LSR_HIP(launch_quick_decode(weight_map, codebooks, L, K, Df, H, W, normalize, eps, ws, out, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_quick_pack_codes(const void* indices, int index_dtype, int64_t N, int K, int quick_dim, uint32_t* packed,
                         void* stream)
{
    if (N < 0 || quick_dim < 0 || index_dtype < LSR_INDEX_F32 || index_dtype > LSR_INDEX_I64) return LSR_EINVAL;
    if (K != 12 || quick_dim > 255) return LSR_EUNSUPPORTED;
    if (N == 0) return LSR_OK;
    if (!indices || !packed || misaligned16(packed)) return LSR_EINVAL;
    LSR_HIP(launch_quick_pack_codes(indices, index_dtype, N, quick_dim > 0 ? quick_dim : 192, packed,
                                    (hipStream_t)stream));
    return LSR_OK;
}

size_t lsr_quick_decode_plan_bytes(int L, int K, int Df, int normalize)
{
    if (codebook_args(L, K, Df) != LSR_OK) return 0;
    return quick_decode_workspace_bytes(L, K, Df, normalize);
}

int lsr_quick_decode_prepare(const float* codebooks, int L, int K, int Df, int normalize, void* plan, void* stream)
{
    LSR_TRY(codebook_args(L, K, Df));
    if (L == 0) return LSR_OK;
    if (!codebooks || !plan) return LSR_EINVAL;
    LSR_HIP(launch_quick_decode_prepare(codebooks, L, K, Df, normalize, plan, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_quick_decode_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int Df, int H,
                         int W, int normalize, float eps, float* out, void* stream)
{
    if (H < 0 || W < 0 || !layout_ok(weight_layout)) return LSR_EINVAL;
    LSR_TRY(codebook_args(L, K, Df));
    if (L == 0 || H == 0 || W == 0) return LSR_OK;
    if (!weight_map || !plan || !out) return LSR_EINVAL;
    const bool hwc = weight_layout == LSR_LAYOUT_HWC;
    // the pixel-major map is read in 32-B pieces by the level-resident kernel (Df <= 512)
    if (hwc && (Df > 512 || misaligned16(weight_map))) return LSR_EUNSUPPORTED;
    LSR_HIP(launch_quick_decode_run(weight_map, L, K, Df, H, W, normalize, eps, plan, out, (hipStream_t)stream, hwc));
    return LSR_OK;
}

size_t lsr_quick_query_plan_bytes(int L, int K, int Df, int n_pos, int n_neg)
{
    if (codebook_args(L, K, Df) != LSR_OK || n_pos < 1 || n_neg < 0 || n_pos + n_neg > 64) return 0;
    return quick_query_plan_bytes(L, K, n_pos, n_neg);
}

int lsr_quick_query_prepare(const float* codebooks, const float* pos, const float* neg, int L, int K, int Df,
                            int n_pos, int n_neg, void* plan, void* stream)
{
    if (n_pos < 1 || n_neg < 0) return LSR_EINVAL;
    LSR_TRY(codebook_args(L, K, Df));
    if (n_pos + n_neg > 64) return LSR_EUNSUPPORTED;
    if (L == 0) return LSR_OK;
    if (!codebooks || !pos || (n_neg > 0 && !neg) || !plan) return LSR_EINVAL;
    LSR_HIP(launch_quick_query_prepare(codebooks, pos, neg, L, K, Df, n_pos, n_neg, plan, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_quick_query_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int n_pos,
                        int n_neg, int H, int W, int mode, float scale, float eps, float* out, void* stream)
{
    if (L < 0 || H < 0 || W < 0 || n_pos < 1 || n_neg < 0 || !layout_ok(weight_layout)) return LSR_EINVAL;
    if (mode != LSR_QUERY_RELEVANCY && mode != LSR_QUERY_COSINE) return LSR_EINVAL;
    const bool relevancy = mode == LSR_QUERY_RELEVANCY;
    // min_j softmax = sigmoid(scale (sim_pos - max_j sim_neg_j)) needs scale >= 0
    if (relevancy && !(scale >= 0.f)) return LSR_EINVAL;
    if (K != 64 || n_pos + n_neg > 64 || (relevancy && n_neg < 1)) return LSR_EUNSUPPORTED;
    if (L == 0 || H == 0 || W == 0) return LSR_OK;
    if (!weight_map || !plan || !out) return LSR_EINVAL;
    const bool hwc = weight_layout == LSR_LAYOUT_HWC;
    // the pixel-major map is read in 16-B pieces
    if (hwc && misaligned16(weight_map)) return LSR_EUNSUPPORTED;
    LSR_HIP(launch_quick_query_run(weight_map, hwc, plan, L, K, n_pos, n_neg, H, W, relevancy, scale, eps, out,
                                   (hipStream_t)stream));
    return LSR_OK;
}

// the semantic entries' shape checks: LSR_EINVAL for a count out of its domain,
// then LSR_EUNSUPPORTED for a shape the kernel does not take
static int semantic_args(int L, int K, int Df, int n_labels, int n_neg)
{
    if (L < 0 || K <= 0 || Df <= 0 || n_labels < 1 || n_neg < 0) return LSR_EINVAL;
    if (K != 64 || (Df % 16) != 0 || (int64_t)n_labels + n_neg > 256) return LSR_EUNSUPPORTED;
    return LSR_OK;
}

size_t lsr_quick_semantic_plan_bytes(int L, int K, int Df, int n_labels, int n_neg)
{
    if (semantic_args(L, K, Df, n_labels, n_neg) != LSR_OK) return 0;
    return quick_semantic_plan_bytes(L, K, n_labels, n_neg);
}

int lsr_quick_semantic_prepare(const float* codebooks, const float* labels, const float* neg, int L, int K, int Df,
                               int n_labels, int n_neg, void* plan, void* stream)
{
    LSR_TRY(semantic_args(L, K, Df, n_labels, n_neg));
    if (L == 0) return LSR_OK;
    if (!codebooks || !labels || (n_neg > 0 && !neg) || !plan) return LSR_EINVAL;
    LSR_HIP(launch_quick_semantic_prepare(codebooks, labels, neg, L, K, Df, n_labels, n_neg, plan,
                                          (hipStream_t)stream));
    return LSR_OK;
}

int lsr_quick_semantic_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int n_labels,
                           int n_neg, int H, int W, float scale, float eps, int32_t* labels_out, float* scores_out,
                           void* stream)
{
    if (H < 0 || W < 0 || !layout_ok(weight_layout)) return LSR_EINVAL;
    // the arg-max of softmax(scale s) is the arg-max of s only for scale >= 0
    if (!(scale >= 0.f)) return LSR_EINVAL;
    LSR_TRY(semantic_args(L, K, 16, n_labels, n_neg));
    if (L == 0 || H == 0 || W == 0) return LSR_OK;
    if (!weight_map || !plan || !labels_out) return LSR_EINVAL;
    const bool hwc = weight_layout == LSR_LAYOUT_HWC;
    // the pixel-major map is read in 16-B pieces
    if (hwc && misaligned16(weight_map)) return LSR_EUNSUPPORTED;
    LSR_HIP(launch_quick_semantic_run(weight_map, hwc, plan, L, K, n_labels, n_neg, H, W, scale, eps, labels_out,
                                      scores_out, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_semantic_merge(const int32_t* labels, const float* scores, int L, int H, int W, int32_t* out, uint8_t* level,
                       void* stream)
{
    if (L < 0 || H < 0 || W < 0) return LSR_EINVAL;
    if (L > 255 || (int64_t)H * W >= (1ll << 31)) return LSR_EUNSUPPORTED;   // the level is written as uint8
    if (L == 0 || H == 0 || W == 0) return LSR_OK;
    if (!labels || !scores || !out) return LSR_EINVAL;
    LSR_HIP(launch_semantic_merge(labels, scores, L, H, W, out, level, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_semantic_confusion(const int32_t* pred, const int32_t* gt, int P, int H, int W, int n_classes, int64_t* counts,
                           void* stream)
{
    if (P < 0 || H < 0 || W < 0 || n_classes < 1) return LSR_EINVAL;
    if (n_classes > 256 || P > 65535 || (int64_t)H * W >= (1ll << 31)) return LSR_EUNSUPPORTED;
    if (P == 0 || H == 0 || W == 0) return LSR_OK;
    if (!pred || !gt || !counts) return LSR_EINVAL;
    LSR_HIP(launch_semantic_confusion(pred, gt, P, H, W, n_classes, counts, (hipStream_t)stream));
    return LSR_OK;
}

size_t lsr_quick_heat_plan_bytes(int L, int K, int Df, int n_pos, int n_neg)
{
    if (codebook_args(L, K, Df) != LSR_OK || L > 3 || n_pos < 1 || n_neg < 0 || n_pos + n_neg > 64) return 0;
    return quick_heat_plan_bytes(L, K, n_pos, n_neg);
}

int lsr_quick_heat_prepare(const float* codebooks, const float* pos, const float* neg, int L, int K, int Df,
                           int n_pos, int n_neg, void* plan, void* stream)
{
    if (n_pos < 1 || n_neg < 0) return LSR_EINVAL;
    LSR_TRY(codebook_args(L, K, Df));
    if (L > 3 || n_pos + n_neg > 64) return LSR_EUNSUPPORTED;
    if (L == 0) return LSR_OK;
    if (!codebooks || !pos || (n_neg > 0 && !neg) || !plan) return LSR_EINVAL;
    LSR_HIP(launch_quick_heat_prepare(codebooks, pos, neg, L, K, Df, n_pos, n_neg, plan, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_quick_heat_run(const float* weight_map, int weight_layout, const void* plan, int L, int K, int n_pos, int n_neg,
                       int H, int W, int mode, float scale, float eps, float* out, void* stream)
{
    if (L < 0 || H < 0 || W < 0 || n_pos < 1 || n_neg < 0 || !layout_ok(weight_layout)) return LSR_EINVAL;
    if (mode != LSR_HEAT_SUMMED_COSINE && mode != LSR_HEAT_MEAN_RELEVANCY) return LSR_EINVAL;
    if (!(scale >= 0.f)) return LSR_EINVAL;
    const bool mean = mode == LSR_HEAT_MEAN_RELEVANCY;
    if (K != 64 || L > 3 || n_pos + n_neg > 64 || (mean && n_neg < 1)) return LSR_EUNSUPPORTED;
    if (L == 0 || H == 0 || W == 0) return LSR_OK;
    if (!weight_map || !plan || !out) return LSR_EINVAL;
    const bool hwc = weight_layout == LSR_LAYOUT_HWC;
    // the pixel-major map is read in 16-B pieces
    if (hwc && misaligned16(weight_map)) return LSR_EUNSUPPORTED;
    LSR_HIP(launch_quick_heat_run(weight_map, hwc, plan, L, K, n_pos, n_neg, H, W, mean, scale, eps, out,
                                  (hipStream_t)stream));
    return LSR_OK;
}

int lsr_heat_frame(const float* maps, const float* stats, const float* rgb, const uint8_t* lut, int planes, int H, int W,
                   int curve, float threshold, float min_range, float alpha, uint8_t* out, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || (curve != LSR_CURVE_UPPER_HALF && curve != LSR_CURVE_POWER4)) return LSR_EINVAL;
    if (!(alpha >= 0.f && alpha <= 1.f)) return LSR_EINVAL;
    if (!heat_frame_shape_ok(planes, H, W)) return LSR_EUNSUPPORTED;
    if (planes == 0 || H == 0 || W == 0) return LSR_OK;
    if (!maps || !stats || !lut || !out) return LSR_EINVAL;
    LSR_HIP(launch_heat_frame(maps, stats, rgb, lut, planes, H, W, curve == LSR_CURVE_POWER4, threshold, min_range,
                              alpha, out, (hipStream_t)stream));
    return LSR_OK;
}

size_t lsr_query_post_workspace_bytes(int planes, int H, int W)
{
    return query_post_workspace_bytes(planes, H, W);
}

int lsr_query_smooth(const float* rel, int planes, int H, int W, int kernel, float* avg, float* blend, float* stats,
                     int64_t* loc, void* workspace, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || kernel < 1 || (kernel & 1) == 0) return LSR_EINVAL;
    if (kernel > 63 || !query_post_shape_ok(planes, H, W)) return LSR_EUNSUPPORTED;
    if (planes == 0 || H == 0 || W == 0) return LSR_OK;
    if (!rel || !stats || !loc || !workspace) return LSR_EINVAL;
    LSR_HIP(launch_query_smooth(rel, planes, H, W, (kernel - 1) / 2, avg, blend, stats, loc, workspace,
                                (hipStream_t)stream));
    return LSR_OK;
}

int lsr_query_mask(const float* blend, const float* stats, const uint8_t* gt_masks, int planes, int n_prompt, int H,
                   int W, float thresh, int smooth_kernel, uint8_t* mask, int64_t* counts, float* masked_sum,
                   void* workspace, void* stream)
{
    if (planes < 0 || H < 0 || W < 0 || smooth_kernel < 1 || (smooth_kernel & 1) == 0) return LSR_EINVAL;
    if (gt_masks && (n_prompt < 1 || planes % n_prompt != 0)) return LSR_EINVAL;
    if (smooth_kernel > 15 || !query_post_shape_ok(planes, H, W)) return LSR_EUNSUPPORTED;
    if (planes == 0 || H == 0 || W == 0) return LSR_OK;
    if (!blend || !stats || !mask || !counts || !masked_sum || !workspace) return LSR_EINVAL;
    LSR_HIP(launch_query_mask(blend, stats, gt_masks, planes, n_prompt, H, W, thresh, (smooth_kernel - 1) / 2, mask,
                              counts, masked_sum, workspace, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_lang_loss_forward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                          const int32_t* seg, const float* features, int S, float* loss, float* pixel_stats,
                          lsr_alloc_fn alloc, void* alloc_ctx, void* stream)
{
    LSR_TRY(lang_loss_args(weight_map, codebooks, K, Df, H, W, seg, features, S));
    if ((!loss && !pixel_stats) || !alloc) return LSR_EINVAL;
    float* ws = (float*)alloc(alloc_ctx, lang_loss_workspace_bytes(S, W, H, nullptr), LSR_BUF_LOSS);
    if (!ws) return LSR_ENOMEM;
    LSR_HIP(launch_lang_loss(weight_map, codebooks, Df, H, W, seg, features, S, nullptr, loss, nullptr, nullptr,
                             pixel_stats, ws, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_lang_loss_backward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                           const int32_t* seg, const float* features, int S, const float* pixel_stats,
                           const float* grad_loss, float* grad_weight_map, float* grad_codebooks, lsr_alloc_fn alloc,
                           void* alloc_ctx, void* stream)
{
    LSR_TRY(lang_loss_args(weight_map, codebooks, K, Df, H, W, seg, features, S));
    if (!grad_loss || !grad_weight_map || !grad_codebooks || !alloc) return LSR_EINVAL;
    float* ws = (float*)alloc(alloc_ctx, lang_loss_workspace_bytes(S, W, H, nullptr), LSR_BUF_LOSS);
    if (!ws) return LSR_ENOMEM;
    LSR_HIP(launch_lang_loss(weight_map, codebooks, Df, H, W, seg, features, S, grad_loss, nullptr, grad_weight_map,
                             grad_codebooks, const_cast<float*>(pixel_stats), ws, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_lang_l1_forward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                        const int32_t* seg, const float* features, int S, int normalize, float* loss,
                        float* pixel_stats, lsr_alloc_fn alloc, void* alloc_ctx, void* stream)
{
    LSR_TRY(lang_loss_args(weight_map, codebooks, K, Df, H, W, seg, features, S));
    if ((!loss && !pixel_stats) || !alloc) return LSR_EINVAL;
    float* ws = (float*)alloc(alloc_ctx, lang_l1_workspace_bytes(Df, W, H), LSR_BUF_LOSS);
    if (!ws) return LSR_ENOMEM;
    LSR_HIP(launch_lang_l1(weight_map, codebooks, Df, H, W, seg, features, S, normalize != 0, nullptr, loss, nullptr,
                           nullptr, pixel_stats, ws, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_lang_l1_backward(const float* weight_map, const float* codebooks, int K, int Df, int H, int W,
                         const int32_t* seg, const float* features, int S, int normalize, const float* pixel_stats,
                         const float* grad_loss, float* grad_weight_map, float* grad_codebooks, lsr_alloc_fn alloc,
                         void* alloc_ctx, void* stream)
{
    LSR_TRY(lang_loss_args(weight_map, codebooks, K, Df, H, W, seg, features, S));
    if (!grad_loss || !grad_weight_map || !grad_codebooks || !alloc) return LSR_EINVAL;
    float* ws = (float*)alloc(alloc_ctx, lang_l1_workspace_bytes(Df, W, H), LSR_BUF_LOSS);
    if (!ws) return LSR_ENOMEM;
    LSR_HIP(launch_lang_l1(weight_map, codebooks, Df, H, W, seg, features, S, normalize != 0, grad_loss, nullptr,
                           grad_weight_map, grad_codebooks, const_cast<float*>(pixel_stats), ws, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_photo_loss_forward(const float* image, const float* gt, int planes, int H, int W, float* out, float* partials,
                           lsr_alloc_fn alloc, void* alloc_ctx, void* stream)
{
    if (!out || !alloc) return LSR_EINVAL;
    LSR_TRY(photo_loss_args(image, gt, planes, H, W));
    void* ws = alloc(alloc_ctx, photo_loss_workspace_bytes(planes, H, W), LSR_BUF_LOSS);
    if (!ws) return LSR_ENOMEM;
    LSR_HIP(launch_photo_loss_fwd(image, gt, planes, H, W, photo_taps(), out, partials, ws, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_photo_loss_backward(const float* image, const float* gt, int planes, int H, int W, const float* partials,
                            const float* grad_out, float* grad_image, void* stream)
{
    if (!partials || !grad_out || !grad_image) return LSR_EINVAL;
    LSR_TRY(photo_loss_args(image, gt, planes, H, W));
    LSR_HIP(launch_photo_loss_bwd(image, gt, planes, H, W, photo_taps(), partials, grad_out, grad_image,
                                  (hipStream_t)stream));
    return LSR_OK;
}

size_t lsr_kmeans_workspace_bytes(int64_t M, int K, int D)
{
    return kmeans_args(M, K, D) != LSR_OK ? 0 : kmeans_workspace_bytes(M, K, D);
}

int lsr_kmeans_prepare(const float* centers, int K, int D, void* workspace, void* stream)
{
    LSR_TRY(kmeans_args(0, K, D));
    if (!centers || !workspace || misaligned16(centers) || misaligned16(workspace)) return LSR_EINVAL;
    LSR_HIP(launch_kmeans_prepare(centers, K, D, workspace, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_kmeans_assign(const float* x, int64_t M, int D, int K, const void* workspace, int32_t* assign, float* dist,
                      float* residual_out, void* stream)
{
    LSR_TRY(kmeans_args(M, K, D));
    if (M == 0) return LSR_OK;
    if (!x || !workspace || !assign || !dist || residual_out == x) return LSR_EINVAL;
    if (misaligned16(x) || misaligned16(workspace) || misaligned16(residual_out)) return LSR_EINVAL;
    LSR_HIP(launch_kmeans_assign(x, (int)M, D, K, workspace, assign, dist, residual_out, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_kmeans_update(const float* x, const int32_t* assign, int64_t M, int D, int K, void* workspace,
                      float* centers_out, int32_t* counts_out, void* stream)
{
    LSR_TRY(kmeans_args(M, K, D));
    if (M == 0) return LSR_OK;
    if (!x || !assign || !workspace || !centers_out || !counts_out) return LSR_EINVAL;
    if (misaligned16(workspace) || misaligned16(centers_out)) return LSR_EINVAL;
    LSR_HIP(launch_kmeans_update(x, assign, (int)M, D, K, workspace, centers_out, counts_out, (hipStream_t)stream));
    return LSR_OK;
}

size_t lsr_mask_nms_workspace_bytes(int N) { return N < 0 || N > LSR_MASK_MAX_N ? 0 : mask_nms_workspace_bytes(N); }

int lsr_mask_pack(const uint8_t* masks, int N, int H, int W, uint64_t* words, int32_t* area, void* stream)
{
    LSR_TRY(mask_args(N, H, W));
    if (N == 0) return LSR_OK;
    if (!masks || !words || !area || misaligned(words, 8) || misaligned(area, 4)) return LSR_EINVAL;
    LSR_HIP(launch_mask_pack(masks, N, H * W, (unsigned long long*)words, area, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_mask_pair_counts(const uint64_t* words, int N, int H, int W, const int32_t* order, int32_t* inter,
                         void* stream)
{
    LSR_TRY(mask_args(N, H, W));
    if (N == 0) return LSR_OK;
    if (!words || !inter || misaligned(words, 8) || misaligned(order, 4) || misaligned(inter, 4)) return LSR_EINVAL;
    LSR_HIP(launch_mask_pairs((const unsigned long long*)words, N, (H * W + 63) / 64, order, inter,
                              (hipStream_t)stream));
    return LSR_OK;
}

int lsr_mask_nms_select(const uint64_t* words, const int32_t* area, int N, int H, int W, const int32_t* order,
                        const uint8_t* conf, double iou_thr, double inner_thr, void* workspace, uint8_t* keep,
                        uint8_t* criteria, int64_t* selected, int32_t* count, void* stream)
{
    LSR_TRY(mask_args(N, H, W));
    if (N == 0) return LSR_OK;
    if (!words || !area || !order || !conf || !workspace || !keep || !selected || !count) return LSR_EINVAL;
    if (misaligned(words, 8) || misaligned(area, 4) || misaligned(order, 4) || misaligned(workspace, 16) ||
        misaligned(selected, 8) || misaligned(count, 4))
        return LSR_EINVAL;
    LSR_HIP(launch_mask_pairs((const unsigned long long*)words, N, (H * W + 63) / 64, order, (int*)workspace,
                              (hipStream_t)stream));
    // torch compares a float32 tensor with a Python scalar in float32; 1 - inner_thr is a Python double first
    LSR_HIP(launch_mask_decide(area, N, order, conf, (float)iou_thr, (float)(1.0 - inner_thr), workspace, keep,
                               criteria, (long long*)selected, count, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_mask_segmaps(const uint64_t* const* words, const int32_t* const* kept, const int32_t* masks,
                     const int32_t* counts, const int32_t* offsets, int H, int W, int index_type, void* out,
                     void* stream)
{
    LSR_TRY(mask_args(0, H, W));
    if (!words || !kept || !masks || !counts || !offsets || !out || misaligned(out, 4)) return LSR_EINVAL;
    if (index_type != LSR_INDEX_F32 && index_type != LSR_INDEX_I32) return LSR_EINVAL;
    for (int l = 0; l < 4; ++l) {
        if (masks[l] < 0 || counts[l] < 0 || offsets[l] < 0) return LSR_EINVAL;
        if (masks[l] > LSR_MASK_MAX_N || counts[l] > LSR_MASK_MAX_N) return LSR_EUNSUPPORTED;
        if (counts[l] > 0 && (!words[l] || !kept[l] || misaligned(words[l], 8) || misaligned(kept[l], 4)))
            return LSR_EINVAL;
    }
    LSR_HIP(launch_mask_segmaps((const unsigned long long* const*)words, kept, masks, counts, offsets, H * W,
                                index_type == LSR_INDEX_I32, out, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_mask_boxes(const uint64_t* words, int N, int H, int W, int32_t* boxes, void* stream)
{
    if (tile_args(N, 0, H, W, 1) != LSR_OK) return LSR_EINVAL;
    if (N == 0) return LSR_OK;
    if (!words || !boxes || misaligned(words, 8) || misaligned(boxes, 4)) return LSR_EINVAL;
    LSR_HIP(launch_mask_boxes((const unsigned long long*)words, N, H, W, boxes, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_clip_tiles(const uint8_t* image, int H, int W, const uint64_t* words, int N, const int32_t* keep,
                   const int32_t* boxes, int n, int S, const void* lut, int out_type, void* out, void* stream)
{
    LSR_TRY(tile_args(N, n, H, W, S));
    if (out_type != LSR_TILE_U8 && out_type != LSR_TILE_UNIT && out_type != LSR_TILE_CLIP) return LSR_EINVAL;
    if (!keep && n > N) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!image || !words || !boxes || !out || (out_type != LSR_TILE_U8 && !lut)) return LSR_EINVAL;
    const uintptr_t elem = out_type == LSR_TILE_UNIT ? 4 : out_type == LSR_TILE_CLIP ? 2 : 1;
    if (misaligned(words, 8) || misaligned(boxes, 4) || misaligned(keep, 4) || misaligned(lut, elem) ||
        misaligned(out, elem))
        return LSR_EINVAL;
    LSR_HIP(launch_clip_tiles(image, H, W, (const unsigned long long*)words, N, keep, boxes, n, S, lut, out_type, out,
                              (hipStream_t)stream));
    return LSR_OK;
}

size_t lsr_densify_workspace_bytes(int64_t N)
{
    return N < 0 || N > LSR_DENSIFY_MAX_ROWS ? 0 : densify_workspace_bytes(N);
}

int lsr_densify_plan(int64_t N, const float* accum, const float* denom, const float* scaling, const float* opacity,
                     float max_grad, float dense_thresh, float min_opacity, int prune_big, float big_thresh,
                     void* workspace, int64_t* counts, void* stream)
{
    // max_grad > 0: a clone's padded gradient is 0 and must stay below it
    if (N < 0 || !(max_grad > 0.f) || !counts) return LSR_EINVAL;
    if (N > LSR_DENSIFY_MAX_ROWS) return LSR_EUNSUPPORTED;
    for (int k = 0; k < LSR_DENSIFY_COUNTS; k++) counts[k] = 0;
    if (N == 0) return LSR_OK;
    if (!accum || !denom || !scaling || !opacity || !workspace) return LSR_EINVAL;
    const DensifyArgs a = {max_grad, dense_thresh, min_opacity, big_thresh, prune_big ? 1 : 0};
    hipStream_t st = (hipStream_t)stream;
    LSR_HIP(launch_densify_plan(N, accum, denom, scaling, opacity, a, workspace, st));
    LSR_HIP(hipMemcpyAsync(counts, densify_counts(N, workspace), LSR_DENSIFY_COUNTS * sizeof(int64_t),
                           hipMemcpyDeviceToHost, st));
    LSR_HIP(hipStreamSynchronize(st));
    return LSR_OK;
}

int lsr_densify_apply(int64_t N, int64_t n_out, const void* workspace, int rest_width, const float* const* src,
                      float* const* dst, const float* noise, void* stream)
{
    if (N < 0 || n_out < 0 || rest_width < 0) return LSR_EINVAL;
    if (N > LSR_DENSIFY_MAX_ROWS || n_out > 2 * LSR_DENSIFY_MAX_ROWS) return LSR_EUNSUPPORTED;
    if (N == 0 || n_out == 0) return LSR_OK;
    if (!workspace || !src || !dst || !noise) return LSR_EINVAL;
    DensifyTable t;
    const int width[LSR_DENSIFY_GROUPS] = {3, 3, rest_width, 1, 3, 4};
    for (int g = 0; g < LSR_DENSIFY_GROUPS; g++) t.width[g] = width[g];
    for (int k = 0; k < 3 * LSR_DENSIFY_GROUPS; k++) {
        const bool param = k < LSR_DENSIFY_GROUPS, empty = width[k % LSR_DENSIFY_GROUPS] == 0;
        // every parameter is read and written (a child's xyz reads scaling and rotation); moments are optional
        if (!empty && ((param && !dst[k]) || (dst[k] && !src[k]))) return LSR_EINVAL;
        t.src[k] = src[k];
        t.dst[k] = empty ? nullptr : dst[k];
    }
    t.noise = noise;
    LSR_HIP(launch_densify_apply(N, n_out, workspace, t, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_reset_opacity(int64_t n, float* opacity, float* exp_avg, float* exp_avg_sq, void* stream)
{
    if (n < 0) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!opacity) return LSR_EINVAL;
    LSR_HIP(launch_reset_opacity(n, opacity, exp_avg, exp_avg_sq, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int64_t step, void* stream)
{
    if (n < 0 || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return LSR_EINVAL;
    if (n == 0) return LSR_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq) return LSR_EINVAL;
    // scalars as torch forms them: Python doubles, rounded once to fp32
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    AdamArgs a;
    a.one_minus_b1 = (float)(1.0 - beta1);
    a.b2 = (float)beta2;
    a.one_minus_b2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.step_size = (float)(lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.weight_decay = (float)weight_decay;
    LSR_HIP(launch_adam(params, grads, exp_avg, exp_avg_sq, n, a, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_topk_code_forward(const float* logits, int64_t N, int L, int K, int k, float* dense, float* sparse_w,
                          void* sparse_idx, int idx_dtype, int level_offset, void* stream)
{
    LSR_TRY(topk_code_args(N, L, K, k));
    if (idx_dtype < LSR_INDEX_F32 || idx_dtype > LSR_INDEX_I64) return LSR_EINVAL;
    if (N == 0) return LSR_OK;
    if (!logits || (!dense && !sparse_w && !sparse_idx)) return LSR_EINVAL;
    LSR_HIP(launch_topk_code_fwd(logits, N, L, K, k, dense, sparse_w, sparse_idx, idx_dtype, level_offset,
                                 (hipStream_t)stream));
    return LSR_OK;
}

int lsr_topk_code_backward(const float* logits, const float* grad_dense, int64_t N, int L, int K, int k,
                           float* grad_logits, void* stream)
{
    return topk_code_backward(logits, grad_dense, N, L, K, k, grad_logits, stream, false);
}

int lsr_topk_code_backward_sparse(const float* logits, const float* grad_weights, int64_t N, int L, int K, int k,
                                  float* grad_logits, void* stream)
{
    return topk_code_backward(logits, grad_weights, N, L, K, k, grad_logits, stream, true);
}

int lsr_knn_dist2(const float* points, int64_t N, float* out, lsr_alloc_fn alloc, void* alloc_ctx, void* stream)
{
    if (N < 0 || N > 0x7fffffffLL) return LSR_EINVAL;
    if (N == 0) return LSR_OK;
    if (!points || !out || !alloc) return LSR_EINVAL;
    size_t sort_temp = 0;
    LSR_HIP(knn_sort_temp_bytes(N, &sort_temp));
    uint8_t* ws = (uint8_t*)alloc(alloc_ctx, knn_workspace_bytes(N, sort_temp), LSR_BUF_KNN);
    if (!ws) return LSR_ENOMEM;
    LSR_HIP(launch_knn_dist2(points, N, out, ws, sort_temp, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_sh_grad_from_views(int64_t N, int M, int sh_degree, const float* means3D, int R, const float* campos,
                           const float* drgb, float* dL_dsh, void* stream)
{
    if (N < 0 || M < 1 || M > 16 || sh_degree < 0 || sh_degree > 3 || (sh_degree + 1) * (sh_degree + 1) > M || R < 0)
        return LSR_EINVAL;
    if (N == 0) return LSR_OK;
    if (!means3D || !dL_dsh || (R > 0 && (!campos || !drgb))) return LSR_EINVAL;
    LSR_HIP(launch_sh_grad_from_views(N, M, sh_degree, means3D, R, campos, drgb, dL_dsh, (hipStream_t)stream));
    return LSR_OK;
}

int lsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream)
{
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return LSR_EINVAL;
    LSR_HIP(launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream));
    return LSR_OK;
}

}  // extern "C"
