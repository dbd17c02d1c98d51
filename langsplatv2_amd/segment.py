"""Segmentation masks and localisation from relevancy maps, fused.

Every caller of get_max_across_quick in the reference post-processes the
(L, Q, H, W) relevancy maps plane by plane (eval_lerf.py:111-156
segmentation_process_cuda, :158-200 localization_process_cuda;
eval_3d_ovs.py:102-107 smooth_cuda, :215-260 its segmentation_process_cuda):

    avg   = AvgPool2d(29, stride 1, padding 14, count_include_pad=False)(v)
    blend = 0.5 * (avg + v)
    o     = clip(2 * (blend - min) / (max - min + 1e-9) - 1, 0, 1)
    mask  = AvgPool2d(7, 1, 3, count_include_pad=False)(o > thresh) > 0.5
    IoU against the annotation mask, a per-level score, the level's argmax;
    for localisation, the maximum of avg and where it lies

The functions here run that on all L * Q planes at once in two HIP tile passes
(csrc/query_post.hip) with a fixed-order reduction after each: four launches,
no host synchronisation, bit-identical results from run to run, and — unlike
the reference, which blends its valid_map in place — the input is never
written.  There is no CPU path and no autograd.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib
from .rasterizer import _stream

_MAX_KERNEL, _MAX_SMOOTH = 63, 15


class SegmentResult(NamedTuple):
    masks: torch.Tensor                 # (L, Q, H, W) uint8
    blend: torch.Tensor                 # (L, Q, H, W) fp32: 0.5 (avg + rel), what the reference leaves in valid_map
    score: torch.Tensor                 # (L, Q) fp32, per `select`
    area: torch.Tensor                  # (L, Q) int64: set pixels of masks
    inter: Optional[torch.Tensor]       # (L, Q) int64 (None without gt_masks)
    union: Optional[torch.Tensor]       # (L, Q) int64 (None without gt_masks)
    iou: Optional[torch.Tensor]         # (L, Q) fp32 = inter / union, nan where the union is empty
    level: torch.Tensor                 # (Q,) int64 = score.argmax(0)


class LocalizeResult(NamedTuple):
    score: torch.Tensor                 # (L, Q) fp32: plane maximum of avg
    yx: torch.Tensor                    # (L, Q, 2) int64: first row-major pixel attaining it
    ties: torch.Tensor                  # (L, Q) int64: how many pixels attain it
    level: torch.Tensor                 # (Q,) int64 = score.argmax(0)
    yx_chosen: torch.Tensor             # (Q, 2) int64: yx at the chosen level


def _check_kernel(what: str, name: str, k, hi: int) -> int:
    if not isinstance(k, int) or isinstance(k, bool) or k < 1 or k > hi or k % 2 == 0:
        raise ValueError(f"{what}: {name} must be an odd integer in 1..{hi}, got {k!r}")
    return k


def _check_rel(what: str, rel: torch.Tensor):
    if not isinstance(rel, torch.Tensor) or rel.dim() != 4:
        raise ValueError(f"{what}: rel must be a (L, Q, H, W) tensor")
    if rel.dtype != torch.float32:
        raise ValueError(f"{what}: rel must be float32, got {rel.dtype}")
    if not rel.is_contiguous():
        raise ValueError(f"{what}: rel must be contiguous")
    if rel.numel() == 0:
        raise ValueError(f"{what}: rel must not be empty, got {tuple(rel.shape)}")
    return tuple(rel.shape)


def _workspace(what: str, lib, planes: int, H: int, W: int, dev) -> torch.Tensor:
    nbytes = int(lib.lsr_query_post_workspace_bytes(planes, H, W))
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported shape ({planes} planes of {H} x {W})")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _smooth(what: str, rel: torch.Tensor, kernel: int, want_avg: bool, want_blend: bool):
    """-> (avg, blend, stats (L, Q, 3) = {min blend, max blend, max avg},
    loc (L, Q, 2) = {argmax index, ties}, workspace)."""
    L, Q, H, W = rel.shape
    dev = rel.device
    lib = _lib.load()
    ws = _workspace(what, lib, L * Q, H, W, dev)
    avg = torch.empty_like(rel) if want_avg else None
    blend = torch.empty_like(rel) if want_blend else None
    stats = torch.empty((L, Q, 3), dtype=torch.float32, device=dev)
    loc = torch.empty((L, Q, 2), dtype=torch.int64, device=dev)
    _lib.check(lib.lsr_query_smooth(rel.data_ptr(), L * Q, H, W, kernel, None if avg is None else avg.data_ptr(),
                                    None if blend is None else blend.data_ptr(), stats.data_ptr(), loc.data_ptr(),
                                    ws.data_ptr(), _stream(dev)), "lsr_query_smooth")
    return avg, blend, stats, loc, ws


@torch.no_grad()
def smooth_maps(rel: torch.Tensor, *, kernel: int = 29, want_avg: bool = True, want_blend: bool = True):
    """rel (L, Q, H, W) contiguous fp32 on the ROCm device -> (avg, blend):
    avg = AvgPool2d(kernel, stride 1, padding (kernel - 1) / 2,
    count_include_pad=False) of every plane and blend = 0.5 * (avg + rel)
    (eval_lerf.py:123-126); either is None when not wanted.  kernel is odd,
    1..63.  rel is not modified."""
    what = "smooth_maps"
    _check_rel(what, rel)
    _check_kernel(what, "kernel", kernel, _MAX_KERNEL)
    if not rel.is_cuda:
        raise RuntimeError(f"{what}: rel must be on the ROCm device (there is no CPU path)")
    avg, blend, _, _, _ = _smooth(what, rel.detach(), kernel, bool(want_avg), bool(want_blend))
    return avg, blend


@torch.no_grad()
def segment_maps(rel: torch.Tensor, thresh: float = 0.4, *, kernel: int = 29, smooth_kernel: int = 7,
                 gt_masks: torch.Tensor | None = None, select: str = "max") -> SegmentResult:
    """The segmentation post-process of the reference on all planes of rel
    (L, Q, H, W) contiguous fp32: blend, normalise to [-1, 1], clip to [0, 1],
    threshold, smooth_kernel x smooth_kernel majority (smooth_cuda), and with
    gt_masks (Q, H, W) uint8 or bool (one annotation mask per prompt, non-zero
    = inside) the intersection, union and IoU of every level's mask.

    select="max" scores a level by the plane maximum of blend
    (eval_lerf.py:147-151); select="masked_mean" by the mean of blend over the
    level's mask for levels 1..L-1, level 0 staying 0 (eval_3d_ovs.py:253-258;
    nan for an empty mask, as there).  level = score.argmax(0).  Everything
    stays on the device; rel is not modified."""
    what = "segment_maps"
    L, Q, H, W = _check_rel(what, rel)
    _check_kernel(what, "kernel", kernel, _MAX_KERNEL)
    _check_kernel(what, "smooth_kernel", smooth_kernel, _MAX_SMOOTH)
    if select not in ("max", "masked_mean"):
        raise ValueError(f"{what}: select must be 'max' or 'masked_mean', got {select!r}")
    if gt_masks is not None:
        if not isinstance(gt_masks, torch.Tensor) or tuple(gt_masks.shape) != (Q, H, W):
            raise ValueError(f"{what}: gt_masks must be (Q, H, W) = ({Q}, {H}, {W})")
        if gt_masks.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{what}: gt_masks must be uint8 or bool, got {gt_masks.dtype}")
        if not gt_masks.is_contiguous():
            raise ValueError(f"{what}: gt_masks must be contiguous")
    if not rel.is_cuda or (gt_masks is not None and not gt_masks.is_cuda):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    if gt_masks is not None and gt_masks.device != rel.device:
        raise ValueError(f"{what}: gt_masks must be on rel's device")
    dev = rel.device
    gt = None if gt_masks is None else (gt_masks.view(torch.uint8) if gt_masks.dtype == torch.bool else gt_masks)
    _, blend, stats, _, ws = _smooth(what, rel.detach(), kernel, False, True)
    masks = torch.empty((L, Q, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty((L, Q, 3), dtype=torch.int64, device=dev)
    msum = torch.empty((L, Q), dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.lsr_query_mask(blend.data_ptr(), stats.data_ptr(), None if gt is None else gt.data_ptr(), L * Q, Q,
                                  H, W, float(thresh), smooth_kernel, masks.data_ptr(), counts.data_ptr(),
                                  msum.data_ptr(), ws.data_ptr(), _stream(dev)), "lsr_query_mask")
    area = counts[..., 0]
    if select == "max":
        score = stats[..., 1]
    else:
        score = msum / area
        score[0] = 0.0
    inter = union = iou = None
    if gt is not None:
        inter, union = counts[..., 1], counts[..., 2]
        iou = inter / union
    return SegmentResult(masks, blend, score, area, inter, union, iou, score.argmax(0))


@torch.no_grad()
def localize_maps(rel: torch.Tensor, *, kernel: int = 29) -> LocalizeResult:
    """The localisation post-process (eval_lerf.py:167-182) on all planes of
    rel (L, Q, H, W) contiguous fp32: score = the maximum of the box-filtered
    map, yx = the first pixel (row-major) attaining it — the reference's
    torch.nonzero(avg == max)[0] — and ties = how many do; level =
    score.argmax(0) and yx_chosen its yx.  The filtered map itself is not
    written.  rel is not modified."""
    what = "localize_maps"
    L, Q, H, W = _check_rel(what, rel)
    _check_kernel(what, "kernel", kernel, _MAX_KERNEL)
    if not rel.is_cuda:
        raise RuntimeError(f"{what}: rel must be on the ROCm device (there is no CPU path)")
    _, _, stats, loc, _ = _smooth(what, rel.detach(), kernel, False, False)
    score = stats[..., 2]
    idx = loc[..., 0]
    yx = torch.stack((idx // W, idx % W), dim=-1)
    level = score.argmax(0)
    yx_chosen = yx[level, torch.arange(Q, device=rel.device)]
    return LocalizeResult(score, yx, loc[..., 1], level, yx_chosen)


def hits(result: LocalizeResult, boxes: Sequence) -> int:
    """The reference's box test (eval_lerf.py:187-199) on the host: boxes[q]
    holds prompt q's boxes as (n, 4) x1 y1 x2 y2 (either corner order); a
    prompt counts once if its chosen point lies inside one of them (bounds
    inclusive).  The reference tests every pixel tied at the maximum; this
    tests the first, which is the only one whenever result.ties is 1."""
    pts = result.yx_chosen.cpu().tolist()
    if len(boxes) != len(pts):
        raise ValueError(f"hits: {len(boxes)} box lists for {len(pts)} prompts")
    acc = 0
    for (y, x), bs in zip(pts, boxes):
        for x1, y1, x2, y2 in torch.as_tensor(bs).reshape(-1, 4).tolist():
            if min(x1, x2) <= x <= max(x1, x2) and min(y1, y2) <= y <= max(y1, y2):
                acc += 1
                break
    return acc
