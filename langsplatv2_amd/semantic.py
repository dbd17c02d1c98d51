"""Open-vocabulary semantic label maps of the quick language path, fused.

The reference's closed-set segmentation path is OpenCLIPNetwork.set_semantics /
get_semantic_map (eval/openclip_encoder.py:75-94): on the decoded, normalised
(L, H, W, Df) map, per level

    output = mm(sem_map[i].view(-1, c), cat([semantic_embeds, neg_embeds]).T)
    label  = argmax(softmax(10 * output)),  -1 where a negative wins

`semantic_maps` computes the same labels from the weight map in one HIP kernel
per frame (csrc/quick_semantic.hip, k_quick_semantic) without the Df-dim map
ever existing, for up to 256 columns, and optionally the softmax value at the
arg-max (the label's confidence).  `merge_levels` picks per pixel the most
confident level (this project's own rule: the reference stops at the per-level
maps), `label_confusion` counts (ground truth, prediction) pairs on the device
and `semantic_scores` turns the counts into IoU / mIoU / pixel accuracy.
Everything that depends only on the codebooks and the label set is prepared
once (`semantic_plan`).  There is no CPU path and no autograd.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import NamedTuple

import torch

from . import _lib
from .lang_loss import _nearest_src
from .query import _check_embeds, _key
from .quick import _OverlapStream, _is_pixel_major
from .rasterizer import _stream

_MAX_COLS = 256   # labels + negatives of one kernel launch (lsr_quick_semantic_run)


class SemanticPlan:
    """The prepared (codebooks, label set) part of the semantic kernel: a device
    buffer written by lsr_quick_semantic_prepare, and the shapes it was made for."""

    __slots__ = ("buf", "L", "K", "Df", "n_labels", "n_neg")

    def __init__(self, buf, L, K, Df, n_labels, n_neg):
        self.buf, self.L, self.K, self.Df, self.n_labels, self.n_neg = buf, L, K, Df, n_labels, n_neg


_PLANS: "OrderedDict[tuple, tuple]" = OrderedDict()
_PLAN_CACHE_SIZE = 8


def _check_set(what, codebooks, label_embeds, neg_embeds):
    if codebooks.dim() != 3:
        raise ValueError(f"{what}: codebooks must be (L, K, Df)")
    L, K, Df = codebooks.shape
    _check_embeds(what, "label_embeds", label_embeds, Df)
    if neg_embeds is not None:
        _check_embeds(what, "neg_embeds", neg_embeds, Df)
    C, N = label_embeds.shape[0], 0 if neg_embeds is None else neg_embeds.shape[0]
    if K != 64 or Df % 16 != 0:
        raise ValueError(f"{what}: K must be 64 and Df a multiple of 16")
    if C < 1:
        raise ValueError(f"{what}: needs at least one label")
    if C + N > _MAX_COLS:
        raise ValueError(f"{what}: {C} labels + {N} negatives = {C + N} columns, more than the {_MAX_COLS} "
                         "one launch takes (C + N <= 256)")
    return L, K, Df, C, N


def semantic_plan(codebooks: torch.Tensor, label_embeds: torch.Tensor,
                  neg_embeds: torch.Tensor | None = None) -> SemanticPlan:
    """The plan for codebooks (L, 64, Df), label embeddings (C, Df) and
    negatives (N, Df) or None, C + N <= 256.  Cached (a small LRU) by storage
    pointer, shape and version counter of all three tensors, as query_plan:
    the same label set across frames reuses its plan."""
    what = "semantic_plan"
    L, K, Df, C, N = _check_set(what, codebooks, label_embeds, neg_embeds)
    tensors = (codebooks, label_embeds) + (() if neg_embeds is None else (neg_embeds,))
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    key = (_key(codebooks), _key(label_embeds), _key(neg_embeds))
    hit = _PLANS.get(key)
    if hit is not None:
        _PLANS.move_to_end(key)
        return hit[1]
    lib = _lib.load()
    dev = codebooks.device
    cb = codebooks.detach().contiguous().float()
    lab = label_embeds.detach().to(dev).contiguous().float()
    neg = None if N == 0 else neg_embeds.detach().to(dev).contiguous().float()
    nbytes = int(lib.lsr_quick_semantic_plan_bytes(L, K, Df, C, N))
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported shape")
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.lsr_quick_semantic_prepare(cb.data_ptr(), lab.data_ptr(), None if neg is None else neg.data_ptr(),
                                              L, K, Df, C, N, buf.data_ptr(), _stream(dev)),
               "lsr_quick_semantic_prepare")
    plan = SemanticPlan(buf, L, K, Df, C, N)
    # the entry keeps the keyed tensors' storage (and their data_ptr) alive
    _PLANS[key] = (tensors, plan)
    while len(_PLANS) > _PLAN_CACHE_SIZE:
        _PLANS.popitem(last=False)
    return plan


def _check_out(what, name, t, shape, dtype, device):
    if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} {shape} tensor on {device}")


@torch.no_grad()
def semantic_maps(weight_map: torch.Tensor, codebooks: torch.Tensor, label_embeds: torch.Tensor,
                  neg_embeds: torch.Tensor | None = None, *, scale: float = 10.0, eps: float = 1e-10,
                  with_scores: bool = False, out=None):
    """weight_map (L*K, H, W) fp32 CUDA (either layout, as for
    decode_language_features), codebooks (L, 64, Df), label_embeds (C, Df),
    neg_embeds (N, Df) or None -> labels (L, H, W) int32: per level and pixel
    the arg-max column of the cosine similarities with cat([label_embeds,
    neg_embeds]), the lowest column on exact ties, -1 where a negative wins
    — the values of get_semantic_map applied to
    decode_language_features(weight_map, codebooks).  with_scores: also
    scores (L, H, W) fp32 = softmax(scale * sim)[arg-max]; the labels are the
    same bits either way.  The embeddings may have any float dtype; they are
    cast to fp32 and used as given (the caller normalises them, as the
    reference does in set_semantics).  C + N <= 256, scale >= 0 (the
    reference's 10).  out: the labels tensor, or (labels, scores) with
    with_scores."""
    what = "semantic_maps"
    if not scale >= 0:
        raise ValueError(f"{what}: scale must be >= 0")
    if weight_map.dim() != 3 or codebooks.dim() != 3:
        raise ValueError(f"{what}: weight_map must be (L*K, H, W) and codebooks (L, K, Df)")
    L, K, Df, C, N = _check_set(what, codebooks, label_embeds, neg_embeds)
    D, H, W = weight_map.shape
    if D != L * K:
        raise ValueError(f"{what}: weight_map has {D} channels, codebooks need L*K = {L * K}")
    if not (weight_map.is_cuda and codebooks.is_cuda):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    dev = weight_map.device
    hwc = _is_pixel_major(weight_map)
    wm = weight_map.detach() if hwc else weight_map.detach().contiguous().float()
    labels = scores = None
    if out is not None:
        labels, scores = out if with_scores else (out, None)
        _check_out(what, "out labels", labels, (L, H, W), torch.int32, dev)
        if with_scores:
            _check_out(what, "out scores", scores, (L, H, W), torch.float32, dev)
    if labels is None:
        labels = torch.empty((L, H, W), dtype=torch.int32, device=dev)
    if with_scores and scores is None:
        scores = torch.empty((L, H, W), dtype=torch.float32, device=dev)
    plan = semantic_plan(codebooks, label_embeds, neg_embeds)
    layout = _lib.LSR_LAYOUT_HWC if hwc else _lib.LSR_LAYOUT_CHW
    _lib.check(_lib.load().lsr_quick_semantic_run(wm.data_ptr(), layout, plan.buf.data_ptr(), L, K, C, N, H, W,
                                                  float(scale), float(eps), labels.data_ptr(),
                                                  scores.data_ptr() if with_scores else None, _stream(dev)),
               "lsr_quick_semantic_run")
    return (labels, scores) if with_scores else labels


def get_semantic_map(weight_map: torch.Tensor, codebooks: torch.Tensor, semantic_embeds: torch.Tensor,
                     neg_embeds: torch.Tensor | None = None, *, eps: float = 1e-10) -> torch.Tensor:
    """The drop-in for OpenCLIPNetwork.get_semantic_map on the decoded map of
    weight_map: (L, H, W) int64 labels, -1 where a negative wins."""
    return semantic_maps(weight_map, codebooks, semantic_embeds, neg_embeds, eps=eps).long()


@torch.no_grad()
def merge_levels(labels: torch.Tensor, scores: torch.Tensor, *, with_level: bool = False):
    """labels (L, H, W) int32 and scores (L, H, W) fp32 of semantic_maps ->
    (H, W) int32: per pixel the label of the level with the largest score, the
    lowest level on ties (scores.argmax(0) and a gather).  with_level: also
    that level, (H, W) uint8.  This rule is this project's own; the reference
    returns the per-level maps only."""
    what = "merge_levels"
    if labels.dim() != 3 or labels.shape != scores.shape:
        raise ValueError(f"{what}: labels and scores must both be (L, H, W)")
    if labels.dtype != torch.int32 or scores.dtype != torch.float32:
        raise ValueError(f"{what}: labels must be int32 and scores float32")
    L, H, W = labels.shape
    if not 1 <= L <= 255:
        raise ValueError(f"{what}: needs 1 to 255 levels")
    if not (labels.is_cuda and scores.is_cuda):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    dev = labels.device
    lab, sco = labels.contiguous(), scores.contiguous()
    out = torch.empty((H, W), dtype=torch.int32, device=dev)
    level = torch.empty((H, W), dtype=torch.uint8, device=dev) if with_level else None
    _lib.check(_lib.load().lsr_semantic_merge(lab.data_ptr(), sco.data_ptr(), L, H, W, out.data_ptr(),
                                              None if level is None else level.data_ptr(), _stream(dev)),
               "lsr_semantic_merge")
    return (out, level) if with_level else out


def _as_int32(t: torch.Tensor) -> torch.Tensor:
    # (a label beyond int32 is outside every class range: clamp, do not wrap)
    if t.dtype != torch.int32:
        t = t.to(torch.int64).clamp(-2, 1 << 20).to(torch.int32)
    return t.contiguous()


@torch.no_grad()
def label_confusion(pred: torch.Tensor, gt: torch.Tensor, n_classes: int) -> torch.Tensor:
    """Confusion counts of predicted label planes against annotated labels.
    pred (H, W) or (P, H, W) integer labels (-1 = no label), gt (Hg, Wg)
    integer labels -> counts (n_classes, n_classes + 1) or (P, n_classes,
    n_classes + 1) int64: counts[..., g, c] pixels with gt == g and pred == c,
    the last column collecting pred == -1.  Pixels whose gt is outside
    [0, n_classes) (ignore labels such as 255 or -1) or whose pred is outside
    [-1, n_classes) are skipped.  A gt of another size is brought to (H, W)
    with the nearest-neighbour source indices of cv2.INTER_NEAREST
    (lang_loss._nearest_src, the rule eval_3d_ovs.py:138 resizes its masks
    with), one gather in torch.  n_classes <= 256."""
    what = "label_confusion"
    if pred.dim() not in (2, 3) or gt.dim() != 2:
        raise ValueError(f"{what}: pred must be (H, W) or (P, H, W) and gt (Hg, Wg)")
    if pred.is_floating_point() or gt.is_floating_point() or pred.dtype == torch.bool or gt.dtype == torch.bool:
        raise ValueError(f"{what}: pred and gt must be integer label tensors")
    C = int(n_classes)
    if not 1 <= C <= 256:
        raise ValueError(f"{what}: n_classes must be 1 to 256")
    if not (pred.is_cuda and gt.is_cuda):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    dev = pred.device
    planes = pred if pred.dim() == 3 else pred[None]
    P, H, W = planes.shape
    if P > 65535:
        raise ValueError(f"{what}: at most 65535 planes")
    g = gt.to(dev)
    if tuple(g.shape) != (H, W) and H > 0 and W > 0:
        if g.shape[0] == 0 or g.shape[1] == 0:
            raise ValueError(f"{what}: gt is empty")
        ys = torch.from_numpy(_nearest_src(H, g.shape[0])).to(dev)
        xs = torch.from_numpy(_nearest_src(W, g.shape[1])).to(dev)
        g = g[ys][:, xs]
    g, p = _as_int32(g), _as_int32(planes)
    counts = torch.zeros((P, C, C + 1), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().lsr_semantic_confusion(p.data_ptr(), g.data_ptr(), P, H, W, C, counts.data_ptr(),
                                                  _stream(dev)), "lsr_semantic_confusion")
    return counts if pred.dim() == 3 else counts[0]


class SemanticScores(NamedTuple):
    iou: torch.Tensor        # (..., C) float64, NaN for a class absent from gt and pred
    miou: torch.Tensor       # (...) float64, over the classes present in gt (NaN if none)
    accuracy: torch.Tensor   # (...) float64, correct / counted pixels (NaN if none)


def semantic_scores(counts: torch.Tensor) -> SemanticScores:
    """counts (..., C, C + 1) of label_confusion -> per-class
    IoU = n_cc / (row_c + col_c - n_cc) (NaN for a class in neither gt nor
    pred), mIoU over the classes present in gt, and pixel accuracy
    sum_c n_cc / sum counts (a pixel predicted -1 counts as wrong).  Plain
    torch, float64, on the counts' device."""
    if counts.dim() < 2 or counts.shape[-1] != counts.shape[-2] + 1:
        raise ValueError("semantic_scores: counts must be (..., C, C + 1)")
    n = counts.to(torch.float64)
    C = n.shape[-2]
    diag = torch.diagonal(n[..., :C], dim1=-2, dim2=-1)
    row = n.sum(-1)                 # pixels annotated c
    col = n[..., :C].sum(-2)        # pixels predicted c
    iou = diag / (row + col - diag)                       # 0 / 0 = NaN
    present = row > 0
    miou = torch.where(present, iou, torch.zeros_like(iou)).sum(-1) / present.sum(-1)
    accuracy = diag.sum(-1) / n.sum((-1, -2))
    return SemanticScores(iou, miou, accuracy)


class QuickSemanticStream(_OverlapStream):
    """Render + label maps over a stream of views, as query.QuickRelevancyStream
    does for the relevancy (the same push / flush contract and stream
    plumbing): the semantic kernel of frame i runs on a side stream while frame
    i + 1 renders; push returns the previous view's labels (L, H, W) int32, or
    (labels, scores) with with_scores.  Each frame's values equal
    semantic_maps(weight map, ...) exactly."""

    def __init__(self, codebooks: torch.Tensor, label_embeds: torch.Tensor, neg_embeds: torch.Tensor | None = None, *,
                 scale: float = 10.0, eps: float = 1e-10, with_scores: bool = False):
        super().__init__(codebooks.device)
        self.codebooks, self.label_embeds, self.neg_embeds = codebooks, label_embeds, neg_embeds
        self.scale, self.eps, self.with_scores = float(scale), float(eps), bool(with_scores)
        # prepared on the caller's stream, which every later side-stream use is ordered after
        semantic_plan(codebooks, label_embeds, neg_embeds)

    def push(self, render_fn):
        return self._unpack(super().push(render_fn))

    def flush(self):
        return self._unpack(super().flush())

    def _unpack(self, out):
        # both maps live in one allocation (one record_stream): plane 0 the labels' bits, plane 1 the scores
        if out is None or not self.with_scores:
            return out
        return out[0], out[1].view(torch.float32)

    def _alloc(self, wm):
        shape = (self.codebooks.shape[0],) + tuple(wm.shape[1:])
        return torch.empty(((2,) if self.with_scores else ()) + shape, dtype=torch.int32, device=wm.device)

    def _run(self, wm, out):
        dst = (out[0], out[1].view(torch.float32)) if self.with_scores else out
        semantic_maps(wm, self.codebooks, self.label_embeds, self.neg_embeds, scale=self.scale, eps=self.eps,
                      with_scores=self.with_scores, out=dst)
