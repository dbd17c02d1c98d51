"""Query heatmap frames for the viewer path, fused.

The reference's two interactive consumers of the quick language map decode all
levels to a (L, 512, H, W) map, reduce it to one map per prompt, copy that to
the host and colour it there:

    backend_renderer.py:204-233   s = sum_l f_l;  sim = (s / (|s| + 1e-10)) . e
        min / max, gates (max < threshold, range < 0.02), "upper half of the
        range" normalisation, COLORMAP_JET, 50/50 blend with the RGB render, uint8
    demo_prompt.py:122-137        get_max_across_quick(...).mean(0)
        min / max, gate (max < 0.22), normalise, ** 4, COLORMAP_JET

`summed_similarity_maps` and `mean_relevancy_maps` take those maps straight
from the weight map in one HIP kernel (csrc/quick_heat.hip, k_quick_heat: all
levels of a pixel at once, |s| from the Cholesky factor of the stacked Gram
matrix of all codebooks); `heat_frames` is the colour tail on the device
(k_heat_frame after lsr_query_smooth's fixed-order min / max: three launches,
no host round trip, bit-identical from run to run).  `QuickHeatStream`
overlaps both with the next view's render.  There is no CPU path and no autograd.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib
from .query import _MAX_COLS, _check_embeds, _chunks, _key
from .quick import _OverlapStream, _is_pixel_major
from .rasterizer import _stream

_MAX_LEVELS = 3
_CURVES = {"upper_half": _lib.LSR_CURVE_UPPER_HALF, "power4": _lib.LSR_CURVE_POWER4}


class HeatPlan:
    """The prepared (codebooks, query set) part of the heat kernel: a device
    buffer written by lsr_quick_heat_prepare, and the shapes it was made for."""

    __slots__ = ("buf", "L", "K", "Df", "n_pos", "n_neg")

    def __init__(self, buf, L, K, Df, n_pos, n_neg):
        self.buf, self.L, self.K, self.Df, self.n_pos, self.n_neg = buf, L, K, Df, n_pos, n_neg


_PLANS: "OrderedDict[tuple, tuple]" = OrderedDict()
_PLAN_CACHE_SIZE = 8


def heat_plan(codebooks: torch.Tensor, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor | None = None) -> HeatPlan:
    """The plan for codebooks (L <= 3, 64, Df), positives (Q, Df) and negatives
    ((N_neg, Df), or None: the summed cosine only), Q + N_neg <= 64.  Cached
    like query.query_plan: by storage pointer, shape and version counter of all
    three tensors.  It is a buffer of its own, not a query plan."""
    what = "heat_plan"
    if codebooks.dim() != 3:
        raise ValueError(f"{what}: codebooks must be (L, K, Df)")
    L, K, Df = codebooks.shape
    _check_embeds(what, "pos_embeds", pos_embeds, Df)
    if neg_embeds is not None:
        _check_embeds(what, "neg_embeds", neg_embeds, Df)
    n_pos, n_neg = pos_embeds.shape[0], 0 if neg_embeds is None else neg_embeds.shape[0]
    if K != 64 or Df % 16 != 0:
        raise ValueError(f"{what}: K must be 64 and Df a multiple of 16")
    if not 1 <= L <= _MAX_LEVELS:
        raise ValueError(f"{what}: needs 1 to {_MAX_LEVELS} levels, got {L}")
    if n_pos < 1 or n_pos + n_neg > _MAX_COLS:
        raise ValueError(f"{what}: needs 1 <= positives and positives + negatives <= {_MAX_COLS}")
    tensors = (codebooks, pos_embeds) + (() if neg_embeds is None else (neg_embeds,))
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    key = (_key(codebooks), _key(pos_embeds), _key(neg_embeds))
    hit = _PLANS.get(key)
    if hit is not None:
        _PLANS.move_to_end(key)
        return hit[1]
    lib = _lib.load()
    dev = codebooks.device
    cb = codebooks.detach().contiguous().float()
    pos = pos_embeds.detach().to(dev).contiguous().float()
    neg = None if n_neg == 0 else neg_embeds.detach().to(dev).contiguous().float()
    nbytes = int(lib.lsr_quick_heat_plan_bytes(L, K, Df, n_pos, n_neg))
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported shape")
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.lsr_quick_heat_prepare(cb.data_ptr(), pos.data_ptr(), None if neg is None else neg.data_ptr(),
                                          L, K, Df, n_pos, n_neg, buf.data_ptr(), _stream(dev)),
               "lsr_quick_heat_prepare")
    plan = HeatPlan(buf, L, K, Df, n_pos, n_neg)
    # the entry keeps the keyed tensors' storage (and their data_ptr) alive
    _PLANS[key] = (tensors, plan)
    while len(_PLANS) > _PLAN_CACHE_SIZE:
        _PLANS.popitem(last=False)
    return plan


def _maps(what, mode, weight_map, codebooks, pos_embeds, neg_embeds, scale, eps, out):
    if weight_map.dim() != 3 or codebooks.dim() != 3:
        raise ValueError(f"{what}: weight_map must be (L*K, H, W) and codebooks (L, K, Df)")
    L, K, Df = codebooks.shape
    D, H, W = weight_map.shape
    if D != L * K:
        raise ValueError(f"{what}: weight_map has {D} channels, codebooks need L*K = {L * K}")
    _check_embeds(what, "pos_embeds" if neg_embeds is not None else "embeds", pos_embeds, Df)
    n_neg = 0
    if neg_embeds is not None:
        _check_embeds(what, "neg_embeds", neg_embeds, Df)
        n_neg = neg_embeds.shape[0]
    Q = pos_embeds.shape[0]
    if K != 64 or Df % 16 != 0:
        raise ValueError(f"{what}: K must be 64 and Df a multiple of 16")
    if not 1 <= L <= _MAX_LEVELS:
        raise ValueError(f"{what}: needs 1 to {_MAX_LEVELS} levels, got {L}")
    if mode == _lib.LSR_HEAT_MEAN_RELEVANCY and not 1 <= n_neg < _MAX_COLS:
        raise ValueError(f"{what}: needs 1 to {_MAX_COLS - 1} negatives")
    if Q < 1:
        raise ValueError(f"{what}: needs at least one positive")
    if not (weight_map.is_cuda and codebooks.is_cuda):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    hwc = _is_pixel_major(weight_map)
    wm = weight_map.detach() if hwc else weight_map.detach().contiguous().float()
    if out is None:
        out = torch.empty((Q, H, W), dtype=torch.float32, device=weight_map.device)
    elif (tuple(out.shape) != (Q, H, W) or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != weight_map.device):
        raise ValueError(f"{what}: out must be a contiguous float32 ({Q}, {H}, {W}) tensor")
    lib = _lib.load()
    layout = _lib.LSR_LAYOUT_HWC if hwc else _lib.LSR_LAYOUT_CHW
    for q0, q1, pos in _chunks(pos_embeds, n_neg):
        plan = heat_plan(codebooks, pos, neg_embeds)
        # the planes of a chunk of the positives are contiguous in out
        _lib.check(lib.lsr_quick_heat_run(wm.data_ptr(), layout, plan.buf.data_ptr(), L, K, q1 - q0, n_neg, H, W,
                                          mode, float(scale), float(eps), out[q0:q1].data_ptr(), _stream(wm.device)),
                   "lsr_quick_heat_run")
    return out


@torch.no_grad()
def summed_similarity_maps(weight_map: torch.Tensor, codebooks: torch.Tensor, embeds: torch.Tensor, *,
                           eps: float = 1e-10, out: torch.Tensor | None = None) -> torch.Tensor:
    """weight_map (L*K, H, W) fp32 on the ROCm device (either layout, as for
    decode_language_features), codebooks (L <= 3, 64, Df), embeds (Q, Df) ->
    (Q, H, W) fp32: the render server's map (backend_renderer.py:204-210), the
    cosine of each embedding with the renormalised sum over levels of the
    normalised decoded features, s = sum_l f_l, s . e / (|s| + eps).  An
    all-zero pixel gives exactly 0.  The embeddings are cast to fp32 and used
    as given (the caller normalises them); more than 64 run in chunks."""
    return _maps("summed_similarity_maps", _lib.LSR_HEAT_SUMMED_COSINE, weight_map, codebooks, embeds, None, 0.0, eps,
                 out)


@torch.no_grad()
def mean_relevancy_maps(weight_map: torch.Tensor, codebooks: torch.Tensor, pos_embeds: torch.Tensor,
                        neg_embeds: torch.Tensor, *, scale: float = 10.0, eps: float = 1e-10,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """(Q, H, W) fp32: query.relevancy_maps(...).mean(0) without the (L, Q, H, W)
    maps (demo_prompt.py:122-123), the levels summed in order and divided by L.
    An all-zero pixel gives exactly 0.5.  scale >= 0 (the reference's 10)."""
    if not scale >= 0:
        raise ValueError("mean_relevancy_maps: scale must be >= 0")
    return _maps("mean_relevancy_maps", _lib.LSR_HEAT_MEAN_RELEVANCY, weight_map, codebooks, pos_embeds, neg_embeds,
                 scale, eps, out)


def jet_lut(device=None) -> torch.Tensor:
    """(256, 3) uint8 RGB: the classic piecewise-linear jet,
    clip(1.5 - |4 x - c|, 0, 1) at x = i / 255 with c = 3, 2, 1 for r, g, b,
    times 255, rounded to nearest.  The reference colours with OpenCV's
    COLORMAP_JET, a 256-entry table shipped inside cv2; cv2 is available neither
    to this project's tests nor in the reference checkout, so that table cannot
    be pinned here: a caller who wants its exact bytes passes their own
    (256, 3) RGB table to heat_frames."""
    x = torch.arange(256, dtype=torch.float64) / 255.0
    rgb = torch.stack([(1.5 - (4.0 * x - c).abs()).clamp(0.0, 1.0) for c in (3.0, 2.0, 1.0)], dim=1)
    lut = (rgb * 255.0 + 0.5).floor().to(torch.uint8)
    return lut if device is None else lut.to(device)


@torch.no_grad()
def heat_frames(maps: torch.Tensor, lut: torch.Tensor, *, rgb: torch.Tensor | None = None,
                curve: str = "upper_half", threshold: float = 0.22, min_range: float = 0.02, alpha: float = 0.5,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """maps (P, H, W) contiguous fp32 on the ROCm device, lut (256, 3) uint8,
    rgb None or (3, H, W) fp32 (the rasterizer's render) -> (P, H, W, 3) uint8
    RGB frames, pixel-major.  Per plane: min and max (fixed-order reduction),
    the gates (max < threshold or max - min < min_range: the whole plane takes
    lut[0]), the curve, the table and, with rgb, rgb * (1 - alpha) + heat / 255
    * alpha clipped to [0, 1] — every step in fp32 (include/lsr.h,
    lsr_heat_frame).  curve "upper_half": clip(2 (x - min) / (max - min + 1e-9)
    - 1, 0, 1); "power4": ((x - min) / (max - min + 1e-8)) ** 4.  The defaults
    are backend_renderer.py's; demo_prompt.py is curve="power4", min_range=0.0,
    rgb=None.  maps is not modified."""
    what = "heat_frames"
    if not isinstance(maps, torch.Tensor) or maps.dim() != 3:
        raise ValueError(f"{what}: maps must be a (P, H, W) tensor")
    if maps.dtype != torch.float32 or not maps.is_contiguous():
        raise ValueError(f"{what}: maps must be contiguous float32")
    if maps.numel() == 0:
        raise ValueError(f"{what}: maps must not be empty, got {tuple(maps.shape)}")
    P, H, W = maps.shape
    if not isinstance(lut, torch.Tensor) or tuple(lut.shape) != (256, 3) or lut.dtype != torch.uint8:
        raise ValueError(f"{what}: lut must be a (256, 3) uint8 tensor")
    if rgb is not None and (not isinstance(rgb, torch.Tensor) or tuple(rgb.shape) != (3, H, W)
                            or rgb.dtype != torch.float32):
        raise ValueError(f"{what}: rgb must be a float32 (3, {H}, {W}) tensor")
    if curve not in _CURVES:
        raise ValueError(f"{what}: curve must be one of {sorted(_CURVES)}, got {curve!r}")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"{what}: alpha must be in [0, 1], got {alpha!r}")
    if not (maps.is_cuda and lut.is_cuda and (rgb is None or rgb.is_cuda)):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    dev = maps.device
    if lut.device != dev or (rgb is not None and rgb.device != dev):
        raise ValueError(f"{what}: lut and rgb must be on maps' device")
    if out is None:
        out = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
    elif (tuple(out.shape) != (P, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f"{what}: out must be a contiguous uint8 ({P}, {H}, {W}, 3) tensor")
    lib = _lib.load()
    nbytes = int(lib.lsr_query_post_workspace_bytes(P, H, W))
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported shape ({P} planes of {H} x {W})")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stats = torch.empty((P, 3), dtype=torch.float32, device=dev)
    loc = torch.empty((P, 2), dtype=torch.int64, device=dev)
    maps, lut = maps.detach(), lut.contiguous()
    rgbc = None if rgb is None else rgb.detach().contiguous()
    # a 1 x 1 box: blend = 0.5 (x + x) = x, so stats = {min x, max x, .} exactly
    _lib.check(lib.lsr_query_smooth(maps.data_ptr(), P, H, W, 1, None, None, stats.data_ptr(), loc.data_ptr(),
                                    ws.data_ptr(), _stream(dev)), "lsr_query_smooth")
    _lib.check(lib.lsr_heat_frame(maps.data_ptr(), stats.data_ptr(), None if rgbc is None else rgbc.data_ptr(),
                                  lut.data_ptr(), P, H, W, _CURVES[curve], float(threshold), float(min_range),
                                  float(alpha), out.data_ptr(), _stream(dev)), "lsr_heat_frame")
    return out


class QuickHeatStream(_OverlapStream):
    """Render + heat frame over a stream of views, with the push / flush
    contract of query.QuickRelevancyStream: push(render_fn) takes a function
    returning (weight_map, rgb) — the quick render's weight map and its
    (3, H, W) image, or None for rgb — and returns the previous view's
    (Q, H, W, 3) uint8 frames (None for the first view); the map and colour
    kernels of frame i run on a side stream while frame i + 1 renders.
    Without neg_embeds the map is summed_similarity_maps (the render server);
    with them mean_relevancy_maps (the prompt demo).  Each frame's bytes equal
    heat_frames(<map function>(weight map, ...), lut, rgb=rgb, ...) exactly."""

    def __init__(self, codebooks: torch.Tensor, embeds: torch.Tensor, lut: torch.Tensor, *,
                 neg_embeds: torch.Tensor | None = None, scale: float = 10.0, eps: float = 1e-10,
                 curve: str = "upper_half", threshold: float = 0.22, min_range: float = 0.02, alpha: float = 0.5):
        super().__init__(codebooks.device)
        self.codebooks, self.embeds, self.neg_embeds, self.lut = codebooks, embeds, neg_embeds, lut
        self.scale, self.eps = float(scale), float(eps)
        self.frame_args = dict(curve=curve, threshold=threshold, min_range=min_range, alpha=alpha)
        # prepared on the caller's stream, which every later side-stream use is ordered after
        for _, _, pos in _chunks(embeds, 0 if neg_embeds is None else neg_embeds.shape[0]):
            heat_plan(codebooks, pos, neg_embeds)

    def _split(self, rendered):
        wm, rgb = rendered
        return wm, (() if rgb is None else (rgb,))

    def _alloc(self, wm):
        return torch.empty((self.embeds.shape[0],) + tuple(wm.shape[1:]) + (3,), dtype=torch.uint8, device=wm.device)

    def _run(self, wm, out, rgb=None):
        if self.neg_embeds is None:
            maps = summed_similarity_maps(wm, self.codebooks, self.embeds, eps=self.eps)
        else:
            maps = mean_relevancy_maps(wm, self.codebooks, self.embeds, self.neg_embeds, scale=self.scale,
                                       eps=self.eps)
        heat_frames(maps, self.lut, rgb=rgb, out=out, **self.frame_args)
