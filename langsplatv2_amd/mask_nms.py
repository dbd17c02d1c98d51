"""SAM mask NMS and segment maps of the preprocess step, on the GPU.

The reference's preprocess.py runs SAM, filters each level's masks with

    masks_default, masks_s, masks_m, masks_l = masks_update(..., iou_thr=0.8, score_thr=0.7, inner_thr=0.5)

(preprocess.py:215-294: a Python double loop over all N (N + 1) / 2 mask pairs,
several full-frame torch reductions per pair on the host), paints each level's
survivors into a segment map (mask2segmap, :304-317) and shifts the levels by
their cumulative lengths (create, :145-157) into the (4, H, W) `<image>_s.npy`
that `lang_loss.language_gt_index` reads.  Here the masks are bit-packed once
(64 pixels per word) and everything between the two networks is HIP
(csrc/mask_nms.hip, C ABI lsr_mask_*): the pair table is integer
popcount(a & b), the decision is one launch with no host read-back, the segment
maps one thread per pixel.  The float arithmetic is the reference's, quirks
included (DESIGN, "Mask NMS and segment maps"); ties in the scores keep input
order (a stable sort).  The 224 x 224 CLIP tiles of the kept masks are cut from
the same packed masks by clip_tiles.py; SAM and OpenCLIP themselves are not
part of this.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

MAX_MASKS = 4096
MAX_PIXELS = 1 << 24
CRIT_IOU, CRIT_CONF, CRIT_INNER_U, CRIT_INNER_L = 1, 2, 4, 8


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _device(who, **tensors):
    for n, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {n} must be a ROCm device tensor (there is no CPU path)")


def _limits(N, H, W, who):
    if N > MAX_MASKS:
        raise ValueError(f"{who}: {N} masks (the kernels take at most {MAX_MASKS})")
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"{who}: a {H} x {W} frame (the kernels take 1 to 2^24 pixels, so every count is exact in fp32)")


@dataclass
class PackedMasks:
    """N bit-packed (H, W) masks: words (N, ceil(H W / 64)) int64, bit b of word w
    is pixel 64 w + b in row-major order (bits past H W are zero); area (N) int32."""
    words: torch.Tensor
    area: torch.Tensor
    H: int
    W: int

    def __len__(self):
        return self.words.shape[0]

    @property
    def device(self):
        return self.words.device

    @staticmethod
    def cat(batches) -> "PackedMasks":
        """Join batches packed one after the other (hundreds of 1080p masks need not be resident as bytes)."""
        batches = list(batches)
        if not batches:
            raise ValueError("PackedMasks.cat: no batches")
        H, W = batches[0].H, batches[0].W
        if any((b.H, b.W) != (H, W) for b in batches):
            raise ValueError("PackedMasks.cat: the batches differ in frame size")
        out = PackedMasks(torch.cat([b.words for b in batches]), torch.cat([b.area for b in batches]), H, W)
        _limits(len(out), H, W, "PackedMasks.cat")
        return out


class NmsResult(NamedTuple):
    selected: torch.Tensor   # (kept,) int64 input indices, descending score
    keep: torch.Tensor       # (N,) bool per rank
    criteria: torch.Tensor   # (N,) uint8 per rank: CRIT_* bits after the fallbacks
    order: torch.Tensor      # (N,) int64 rank -> input index
    inter: torch.Tensor      # (N, N) int32 in rank order, upper triangle and diagonal


def pack_masks(masks: torch.Tensor) -> PackedMasks:
    """Bit-pack (N, H, W) uint8 or bool masks (nonzero = set); other dtypes are compared with 0 first."""
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3:
        raise ValueError("pack_masks: masks must be a 3-D tensor (N, H, W), got "
                         f"{tuple(masks.shape) if isinstance(masks, torch.Tensor) else type(masks).__name__}")
    _device("pack_masks", masks=masks)
    N, H, W = masks.shape
    _limits(N, H, W, "pack_masks")
    if masks.dtype == torch.bool:
        m = masks.contiguous().view(torch.uint8)
    elif masks.dtype == torch.uint8:
        m = masks.contiguous()
    else:
        m = (masks != 0).view(torch.uint8)
    words = torch.empty((N, (H * W + 63) // 64), dtype=torch.int64, device=m.device)
    area = torch.empty(N, dtype=torch.int32, device=m.device)
    if N:
        _lib.check(_lib.load().lsr_mask_pack(m.data_ptr(), N, H, W, words.data_ptr(), area.data_ptr(),
                                             _stream(m.device)), "lsr_mask_pack")
    return PackedMasks(words, area, H, W)


def _packed(x, who) -> PackedMasks:
    if isinstance(x, PackedMasks):
        _device(who, masks=x.words, area=x.area)
        _limits(len(x), x.H, x.W, who)
        if (x.words.dtype != torch.int64 or tuple(x.words.shape) != (len(x), (x.H * x.W + 63) // 64)
                or x.area.dtype != torch.int32 or tuple(x.area.shape) != (len(x),)):
            raise ValueError(f"{who}: PackedMasks must hold (N, ceil(H W / 64)) int64 words and (N,) int32 areas")
        if x.words.is_contiguous() and x.area.is_contiguous():
            return x
        return PackedMasks(x.words.contiguous(), x.area.contiguous(), x.H, x.W)
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"{who}: masks must be a PackedMasks or a 3-D tensor (N, H, W)")
    _device(who, masks=x)
    return pack_masks(x)


def mask_pair_counts(packed: PackedMasks, order: torch.Tensor | None = None) -> torch.Tensor:
    """(N, N) int32: entry [i][j], i <= j, is the number of pixels masks order[i]
    and order[j] share (order None: input order); below the diagonal 0.  Exact."""
    packed = _packed(packed, "mask_pair_counts")
    N = len(packed)
    inter = torch.empty((N, N), dtype=torch.int32, device=packed.device)
    if N == 0:
        return inter
    o = None
    if order is not None:
        if order.dim() != 1 or order.shape[0] != N:
            raise ValueError(f"mask_pair_counts: order must be ({N},), got {tuple(order.shape)}")
        _device("mask_pair_counts", order=order)
        o = order.to(torch.int32).contiguous()
    _lib.check(_lib.load().lsr_mask_pair_counts(packed.words.data_ptr(), N, packed.H, packed.W,
                                                o.data_ptr() if o is not None else None, inter.data_ptr(),
                                                _stream(packed.device)), "lsr_mask_pair_counts")
    return inter


def mask_nms(masks, scores: torch.Tensor, iou_thr: float = 0.7, score_thr: float = 0.1, inner_thr: float = 0.2,
             return_detail: bool = False, **kwargs):
    """preprocess.py:215-279: the input indices of the masks that survive, as a
    LongTensor in descending score order.  masks: (N, H, W) or PackedMasks;
    scores: (N,) float32 or float64, compared with score_thr in their own dtype.
    With return_detail an NmsResult."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 1:
        raise ValueError("mask_nms: scores must be a 1-D tensor")
    if not isinstance(masks, PackedMasks) and (not isinstance(masks, torch.Tensor) or masks.dim() != 3):
        raise ValueError("mask_nms: masks must be a PackedMasks or a 3-D tensor (N, H, W)")
    N = len(masks)
    if scores.shape[0] != N:
        raise ValueError(f"mask_nms: {N} masks but {scores.shape[0]} scores")
    if not scores.dtype.is_floating_point:
        raise ValueError(f"mask_nms: scores must be floating point, got {scores.dtype}")
    packed = _packed(masks, "mask_nms")
    _device("mask_nms", scores=scores)
    dev = packed.device
    if N == 0:
        sel = torch.empty(0, dtype=torch.int64, device=dev)
        if not return_detail:
            return sel
        return NmsResult(sel, torch.empty(0, dtype=torch.bool, device=dev), torch.empty(0, dtype=torch.uint8, device=dev),
                         sel.clone(), torch.empty((0, 0), dtype=torch.int32, device=dev))
    lib = _lib.load()
    # plumbing: the stable sort and the confidence compare, in the scores' dtype
    ranked, idx = torch.sort(scores.detach().to(dev), dim=0, descending=True, stable=True)
    conf = (ranked > score_thr).to(torch.uint8)
    order = idx.to(torch.int32)
    ws = torch.empty(lib.lsr_mask_nms_workspace_bytes(N), dtype=torch.uint8, device=dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    crit = torch.empty(N, dtype=torch.uint8, device=dev)
    selected = torch.empty(N, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.lsr_mask_nms_select(packed.words.data_ptr(), packed.area.data_ptr(), N, packed.H, packed.W,
                                       order.data_ptr(), conf.data_ptr(), float(iou_thr), float(inner_thr),
                                       ws.data_ptr(), keep.data_ptr(), crit.data_ptr(), selected.data_ptr(),
                                       count.data_ptr(), _stream(dev)), "lsr_mask_nms_select")
    sel = selected[:int(count.item())]
    if not return_detail:
        return sel
    inter = ws[:4 * N * N].view(torch.int32).view(N, N)
    return NmsResult(sel, keep.bool(), crit, idx, inter)


def masks_update(*levels, device="cuda", **kwargs):
    """Drop-in for preprocess.py:281-294: each argument is one level's list of SAM
    dicts (`segmentation`, `predicted_iou`, `stability_score`); returns a tuple of
    the filtered lists, members in their original order.  kwargs go to mask_nms."""
    out = ()
    for lvl in levels:
        if len(lvl) == 0:
            out += ([],)
            continue
        seg = torch.from_numpy(np.stack([np.asarray(m["segmentation"]) for m in lvl], axis=0)).to(device)
        iou_pred = np.stack([m["predicted_iou"] for m in lvl], axis=0)
        stability = np.stack([m["stability_score"] for m in lvl], axis=0)
        scores = torch.from_numpy(np.atleast_1d(stability * iou_pred)).to(device)
        kept = set(mask_nms(seg, scores, **kwargs).tolist())
        out += ([m for i, m in enumerate(lvl) if i in kept],)
    return out


def build_seg_maps(levels, keeps=None, dtype=torch.float32):
    """The (4, H, W) segment maps of `<image>_s.npy` and the four level lengths.

    levels: up to four of (N_l, H, W) masks, PackedMasks or None (default, s, m,
    l); keeps[l]: the indices of level l's masks that stay, in list order (None:
    all of them).  A pixel's value in level l is the highest position in keeps[l]
    whose mask covers it (later masks win, as mask2segmap's loop) plus the lengths
    of the levels before it (create's offsets); -1 where no mask does.
    dtype float32 is what the file holds, int32 what language_gt_index returns."""
    if dtype not in (torch.float32, torch.int32):
        raise ValueError(f"build_seg_maps: dtype must be float32 or int32, got {dtype}")
    levels = list(levels)
    if not 1 <= len(levels) <= 4:
        raise ValueError(f"build_seg_maps: {len(levels)} levels (1 to 4)")
    keeps = [None] * len(levels) if keeps is None else list(keeps)
    if len(keeps) != len(levels):
        raise ValueError(f"build_seg_maps: {len(levels)} levels but {len(keeps)} keep lists")
    packed = [None if lv is None else _packed(lv, "build_seg_maps") for lv in levels]
    sized = [p for p in packed if p is not None]
    if not sized:
        raise ValueError("build_seg_maps: no level gives the frame size")
    H, W, dev = sized[0].H, sized[0].W, sized[0].device
    if any((p.H, p.W) != (H, W) for p in sized):
        raise ValueError("build_seg_maps: the levels differ in frame size")
    _limits(0, H, W, "build_seg_maps")
    p4 = ctypes.c_void_p * 4
    i4 = ctypes.c_int32 * 4
    words, kept, nmask, counts, offsets = p4(), p4(), i4(), i4(), i4()
    hold, lengths, total = [], [], 0
    for l in range(4):
        p = packed[l] if l < len(packed) else None
        n = 0
        if p is not None and len(p):
            k = keeps[l]
            if k is None:
                k = torch.arange(len(p), dtype=torch.int32, device=dev)
            else:
                k = torch.as_tensor(k)
                if k.dim() != 1 or k.dtype.is_floating_point:
                    raise ValueError(f"build_seg_maps: keeps[{l}] must be a 1-D index tensor")
                if k.shape[0] > MAX_MASKS:
                    raise ValueError(f"build_seg_maps: keeps[{l}] has {k.shape[0]} entries (at most {MAX_MASKS})")
                k = k.to(device=dev, dtype=torch.int32).contiguous()
            n = k.shape[0]
            if n:
                hold.append(k)
                words[l], kept[l], nmask[l] = p.words.data_ptr(), k.data_ptr(), len(p)
        counts[l], offsets[l] = n, total
        lengths.append(n)
        total += n
    out = torch.empty((4, H, W), dtype=dtype, device=dev)
    index_type = _lib.LSR_INDEX_I32 if dtype == torch.int32 else _lib.LSR_INDEX_F32
    _lib.check(_lib.load().lsr_mask_segmaps(words, kept, nmask, counts, offsets, H, W, index_type, out.data_ptr(),
                                            _stream(dev)), "lsr_mask_segmaps")
    return out, lengths
