"""The CLIP input tiles of the preprocess step's kept SAM masks, on the GPU.

The reference's mask2segmap (preprocess.py:304-317) loops over the kept masks on
the host: get_seg_img (:191-196) copies the frame, blacks out what the mask does
not cover and crops to SAM's `bbox`; pad_img (:198-206) centres the crop in a
square; cv2.resize brings it to 224 x 224.  The stack is divided by 255 (:315),
and encode_image (:105-107) normalises with the CLIP mean and std (:42-43) and
casts to half.  Here one HIP kernel (csrc/clip_tiles.hip, C ABI lsr_clip_tiles)
writes the tiles in any of these three forms straight from the bit-packed masks
of mask_nms.py, so SAM's output reaches CLIP's input without leaving the device:

    pack_masks -> mask_nms -> build_seg_maps and clip_tiles

The resize is OpenCV's 8-bit INTER_LINEAR arithmetic in integers, written from
its source; it has not been compared with a cv2 build (DESIGN, "CLIP tiles").
Two deviations from the reference: a crop of no pixels gives an all-zero tile
(cv2.resize raises), and a negative box origin is clamped to the frame (numpy
slicing would wrap it); SAM yields neither.  There is no CPU path.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .mask_nms import MAX_MASKS, PackedMasks, _device, _packed, _stream, build_seg_maps, mask_nms

MAX_SIDE = 1024
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)    # preprocess.py:42
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)    # preprocess.py:43
LEVEL_NAMES = ("default", "s", "m", "l")
_OUT = {"u8": (_lib.LSR_TILE_U8, torch.uint8), "unit": (_lib.LSR_TILE_UNIT, torch.float32),
        "clip": (_lib.LSR_TILE_CLIP, torch.float16)}
_LUTS = {}


def tile_lut(out: str, mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """The (3, 256) table a pixel value goes through, by torch's own float32 ops on
    the host as the reference's: "unit" v / 255.0 (preprocess.py:315), "clip"
    ((v / 255.0) - mean[c]) / std[c] cast to half (torchvision's Normalize, .half())."""
    if out not in ("unit", "clip"):
        raise ValueError(f"tile_lut: out must be 'unit' or 'clip', got {out!r}")
    unit = (torch.arange(256, dtype=torch.uint8) / 255.0).expand(3, 256)
    if out == "unit":
        return unit.contiguous()
    m = torch.as_tensor(mean, dtype=torch.float32).reshape(-1)
    s = torch.as_tensor(std, dtype=torch.float32).reshape(-1)
    if m.shape[0] != 3 or s.shape[0] != 3:
        raise ValueError("tile_lut: mean and std must hold 3 values each")
    return ((unit - m[:, None]) / s[:, None]).half().contiguous()


def _lut_on(dev, out, mean, std):
    key = (str(dev), out) + (() if out == "unit" else (tuple(float(v) for v in torch.as_tensor(mean).reshape(-1)),
                                                         tuple(float(v) for v in torch.as_tensor(std).reshape(-1))))
    if key not in _LUTS:
        _LUTS[key] = tile_lut(out, mean, std).to(dev)
    return _LUTS[key]


def mask_boxes(masks) -> torch.Tensor:
    """(N, 4) int32 x, y, w, h: the tight extents of each mask ((N, H, W) or
    PackedMasks), covering every set pixel; an empty mask gives 0, 0, 0, 0."""
    packed = _packed(masks, "mask_boxes")
    N = len(packed)
    boxes = torch.empty((N, 4), dtype=torch.int32, device=packed.device)
    if N:
        _lib.check(_lib.load().lsr_mask_boxes(packed.words.data_ptr(), N, packed.H, packed.W, boxes.data_ptr(),
                                              _stream(packed.device)), "lsr_mask_boxes")
    return boxes


def clip_tiles(image: torch.Tensor, masks, boxes=None, keep=None, out: str = "clip", size: int = 224,
               mean=CLIP_MEAN, std=CLIP_STD) -> torch.Tensor:
    """One size x size tile per kept mask: the frame where the mask covers it, black
    elsewhere, cropped to the mask's box, centred in a square and resized.

    image: (H, W, 3) uint8 on the device, in the channel order wanted out.
    masks: (N, H, W) or PackedMasks.  boxes: (N, 4) integer x, y, w, h per mask
    (SAM's `bbox` after np.int32; None: mask_boxes).  keep: (n,) mask indices, tile
    t is mask keep[t] (None: every mask in order).  out: "u8" (n, size, size, 3)
    uint8, the stack of the reference's resized crops; "unit" (n, 3, size, size)
    float32 = u8 / 255.0, mask2segmap's seg_imgs; "clip" (n, 3, size, size) float16
    = half((u8 / 255.0 - mean[c]) / std[c]), what encode_image hands the model."""
    if out not in _OUT:
        raise ValueError(f"clip_tiles: out must be one of {sorted(_OUT)}, got {out!r}")
    if not isinstance(size, int) or not 1 <= size <= MAX_SIDE:
        raise ValueError(f"clip_tiles: size must be an integer in 1 .. {MAX_SIDE}, got {size!r}")
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError("clip_tiles: image must be a 3-D tensor (H, W, 3), got "
                         f"{tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__}")
    if image.dtype != torch.uint8:
        raise ValueError(f"clip_tiles: image must be uint8, got {image.dtype}")
    if not isinstance(masks, PackedMasks) and (not isinstance(masks, torch.Tensor) or masks.dim() != 3):
        raise ValueError("clip_tiles: masks must be a PackedMasks or a 3-D tensor (N, H, W)")
    _device("clip_tiles", image=image)
    packed = _packed(masks, "clip_tiles")
    N, H, W, dev = len(packed), packed.H, packed.W, packed.device
    if tuple(image.shape[:2]) != (H, W):
        raise ValueError(f"clip_tiles: image is {image.shape[0]} x {image.shape[1]} but the masks are {H} x {W}")
    if image.device != dev:
        raise ValueError(f"clip_tiles: image is on {image.device} but the masks are on {dev}")
    if boxes is None:
        boxes = mask_boxes(packed)
    else:
        if not isinstance(boxes, torch.Tensor) or tuple(boxes.shape) != (N, 4) or boxes.dtype.is_floating_point:
            raise ValueError(f"clip_tiles: boxes must be an ({N}, 4) integer tensor of x, y, w, h")
        _device("clip_tiles", boxes=boxes)
        boxes = boxes.to(torch.int32).contiguous()
    k = None
    n = N
    if keep is not None:
        k = torch.as_tensor(keep)
        if k.dim() != 1 or k.dtype.is_floating_point or k.dtype == torch.bool:
            raise ValueError("clip_tiles: keep must be a 1-D index tensor")
        if k.shape[0] > MAX_MASKS:
            raise ValueError(f"clip_tiles: keep has {k.shape[0]} entries (at most {MAX_MASKS})")
        k = k.to(device=dev, dtype=torch.int32).contiguous()
        n = k.shape[0]
    out_type, dtype = _OUT[out]
    shape = (n, size, size, 3) if out == "u8" else (n, 3, size, size)
    tiles = torch.empty(shape, dtype=dtype, device=dev)
    if n == 0:
        return tiles
    lut = None if out == "u8" else _lut_on(dev, out, mean, std)
    image = image.contiguous()
    _lib.check(_lib.load().lsr_clip_tiles(image.data_ptr(), H, W, packed.words.data_ptr(), N,
                                          k.data_ptr() if k is not None else None, boxes.data_ptr(), n, size,
                                          lut.data_ptr() if lut is not None else None, out_type, tiles.data_ptr(),
                                          _stream(dev)), "lsr_clip_tiles")
    return tiles


def _sam_level(masks, device):
    """One level's SAM dicts as packed masks and (N, 4) int32 boxes on the device."""
    seg = torch.from_numpy(np.stack([np.asarray(m["segmentation"]) for m in masks], axis=0)).to(device)
    boxes = torch.from_numpy(np.stack([np.int32(m["bbox"]) for m in masks], axis=0).reshape(-1, 4)).to(device)
    return _packed(seg, "clip_tiles"), boxes


def _frame(image, device):
    if isinstance(image, torch.Tensor):
        return image.to(device)
    return torch.from_numpy(np.ascontiguousarray(image)).to(device)


def mask2segmap(masks, image, device="cuda", out: str = "unit", **kwargs):
    """Drop-in for the reference's inner mask2segmap (preprocess.py:304-317): masks is
    a list of SAM dicts (`segmentation`, `bbox`), image an (H, W, 3) uint8 array.
    Returns (seg_imgs, seg_map): the tiles on the device in the form `out` and the
    (H, W) int32 numpy map, -1 where no mask covers a pixel, later masks winning.
    kwargs go to clip_tiles (size, mean, std)."""
    if len(masks) == 0:
        raise ValueError("mask2segmap: no masks (the reference skips an empty level)")
    packed, boxes = _sam_level(masks, device)
    tiles = clip_tiles(_frame(image, packed.device), packed, boxes, out=out, **kwargs)
    seg, _ = build_seg_maps([packed], dtype=torch.int32)
    return tiles, seg[0].cpu().numpy()


def segment_tiles_and_maps(image, levels, out: str = "clip", device="cuda", size: int = 224, mean=CLIP_MEAN,
                           std=CLIP_STD, **nms_kwargs):
    """The body of the reference's sam_encoder after mask_generator.generate
    (preprocess.py:300-329) for up to four levels (default, s, m, l) of SAM dicts
    (`segmentation`, `bbox`, `predicted_iou`, `stability_score`): mask_nms per
    level (nms_kwargs are its thresholds), the tiles of the survivors in their
    original order, and the segment maps.  Each level is packed once.  Returns
    (tiles, seg_maps, lengths): tiles maps the level's name to its tiles in the
    form `out` (an empty level has no entry, as in the reference), seg_maps is the
    (4, H, W) float32 device tensor of `<image>_s.npy` with create's offsets
    (:145-157), lengths the four kept counts."""
    levels = list(levels)
    if not 1 <= len(levels) <= 4:
        raise ValueError(f"segment_tiles_and_maps: {len(levels)} levels (1 to 4)")
    packs, keeps, tiles = [], [], {}
    frame = None
    for name, lvl in zip(LEVEL_NAMES, levels):
        if lvl is None or len(lvl) == 0:
            packs.append(None)
            keeps.append(None)
            continue
        packed, boxes = _sam_level(lvl, device)
        if frame is None:
            frame = _frame(image, packed.device)
        scores = np.stack([m["stability_score"] for m in lvl]) * np.stack([m["predicted_iou"] for m in lvl])
        kept = mask_nms(packed, torch.from_numpy(np.atleast_1d(scores)).to(packed.device), **nms_kwargs)
        kept = torch.sort(kept).values   # masks_update keeps the list's order
        packs.append(packed)
        keeps.append(kept)
        if kept.shape[0]:
            tiles[name] = clip_tiles(frame, packed, boxes, keep=kept, out=out, size=size, mean=mean, std=std)
    if frame is None:
        raise ValueError("segment_tiles_and_maps: every level is empty")
    seg_maps, lengths = build_seg_maps(packs, keeps)
    return tiles, seg_maps, lengths
