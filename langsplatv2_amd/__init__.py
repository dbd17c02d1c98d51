"""langsplatv2_amd — MI355X-native (gfx950 HIP) differentiable tile rasterizer
for high-dimensional language Gaussian splatting.

The drop-in operator surface lives in `diff_gaussian_rasterization` (a thin
top-level package re-exporting `langsplatv2_amd.rasterizer`), so LangSplatV2's
gaussian_renderer/__init__.py and train.py run unchanged.  Compute is in
liblsr.so (C ABI: include/lsr.h).
"""
from ._lib import deterministic, set_deterministic  # noqa: F401
from .clip_tiles import clip_tiles, mask2segmap, mask_boxes, segment_tiles_and_maps  # noqa: F401
from .codebook_init import (ResidualVectorQuantizationWithClustering, assign_codes, fit_codebooks,  # noqa: F401
                            kmeans_step, quantize)
from .densify import (DensifyResult, densify_and_prune, densify_and_prune_torch, densify_tensors,  # noqa: F401
                      reset_opacity)
from .heatmap import (QuickHeatStream, heat_frames, heat_plan, jet_lut, mean_relevancy_maps,  # noqa: F401
                      summed_similarity_maps)
from .lang_loss import language_l1_loss  # noqa: F401
from .mask_nms import (NmsResult, PackedMasks, build_seg_maps, mask_nms, mask_pair_counts,  # noqa: F401
                       masks_update, pack_masks)
from .photo_loss import l1_ssim, photometric_loss  # noqa: F401
from .query import QuickRelevancyStream, query_plan, relevancy_maps, similarity_maps  # noqa: F401
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer,  # noqa: F401
                         rasterize_gaussians)
from .semantic import (QuickSemanticStream, SemanticScores, get_semantic_map, label_confusion,  # noqa: F401
                       merge_levels, semantic_maps, semantic_plan, semantic_scores)
from .segment import (LocalizeResult, SegmentResult, hits, localize_maps, segment_maps,  # noqa: F401
                      smooth_maps)

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "deterministic",
           "set_deterministic", "relevancy_maps", "similarity_maps", "query_plan", "QuickRelevancyStream",
           "smooth_maps", "segment_maps", "localize_maps", "hits", "SegmentResult", "LocalizeResult",
           "summed_similarity_maps", "mean_relevancy_maps", "heat_frames", "jet_lut", "heat_plan", "QuickHeatStream",
           "photometric_loss", "l1_ssim", "language_l1_loss", "densify_tensors", "densify_and_prune", "densify_and_prune_torch", "reset_opacity",
           "DensifyResult", "assign_codes", "kmeans_step", "quantize", "fit_codebooks",
           "ResidualVectorQuantizationWithClustering", "pack_masks", "mask_pair_counts", "mask_nms", "masks_update",
           "build_seg_maps", "PackedMasks", "NmsResult", "mask_boxes", "clip_tiles", "mask2segmap",
           "segment_tiles_and_maps", "semantic_maps", "semantic_plan", "get_semantic_map", "merge_levels",
           "label_confusion", "semantic_scores", "SemanticScores", "QuickSemanticStream"]
