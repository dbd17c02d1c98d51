"""Text-query relevancy maps of the quick language path, fused.

The reference decodes the rendered weight map to a normalised (L, H, W, Df)
feature map (eval_lerf.py:210-220) and always hands it to
OpenCLIPNetwork.get_max_across_quick (eval/openclip_encoder.py:114-139;
callers eval_lerf.py:113,160, eval_3d_ovs.py:112,217, demo_prompt.py:122):

    sim = einsum('nqc,pc->nqp', sem_map_flat, cat([pos_embeds, neg_embeds]))
    softmax(10 * stack([pos, neg_j]))[..., 0].min over j  ->  (L, Q, H, W)

`relevancy_maps` computes the same values from the weight map in one HIP
kernel per frame (csrc/quick_query.hip, k_quick_query) without the Df-dim map ever
existing: per level f . e = w^T (CB e), |f| = |L^T w| with the Cholesky factor
of the codebook Gram matrix, and the 2-way softmax + min over the negatives is
sigmoid(scale * (sim_pos - max_j sim_neg_j)).  Everything that depends only on
the codebooks and the query set is prepared once (`query_plan`).  There is no
CPU path and no autograd.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib
from .quick import _OverlapStream, _is_pixel_major
from .rasterizer import _stream

_MAX_COLS = 64   # positives + negatives of one kernel launch (lsr_quick_query_run)


class QueryPlan:
    """The prepared (codebooks, query set) part of the query kernel: a device
    buffer written by lsr_quick_query_prepare, and the shapes it was made for."""

    __slots__ = ("buf", "L", "K", "Df", "n_pos", "n_neg")

    def __init__(self, buf, L, K, Df, n_pos, n_neg):
        self.buf, self.L, self.K, self.Df, self.n_pos, self.n_neg = buf, L, K, Df, n_pos, n_neg


_PLANS: "OrderedDict[tuple, tuple]" = OrderedDict()
_PLAN_CACHE_SIZE = 8


def _key(t: torch.Tensor | None):
    if t is None:
        return None
    return (t.data_ptr(), t.device, t.dtype, tuple(t.shape), tuple(t.stride()), t._version)


def _check_embeds(what: str, name: str, e: torch.Tensor, Df: int):
    if e.dim() != 2 or e.shape[1] != Df:
        raise ValueError(f"{what}: {name} must be (n, Df = {Df}), got {tuple(e.shape)}")
    if not e.is_floating_point():
        raise ValueError(f"{what}: {name} must be a floating-point tensor")


def query_plan(codebooks: torch.Tensor, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor | None) -> QueryPlan:
    """The plan for codebooks (L, 64, Df), positives (Q, Df) and negatives
    (N_neg, Df), or None: cosine maps only), Q + N_neg <= 64.  Cached (a small
    LRU) by storage pointer, shape and version counter of all three tensors:
    the same prompt across frames reuses its plan, an optimizer step on the
    codebooks or a new prompt prepares a new one."""
    what = "query_plan"
    if codebooks.dim() != 3:
        raise ValueError(f"{what}: codebooks must be (L, K, Df)")
    L, K, Df = codebooks.shape
    _check_embeds(what, "pos_embeds", pos_embeds, Df)
    if neg_embeds is not None:
        _check_embeds(what, "neg_embeds", neg_embeds, Df)
    n_pos, n_neg = pos_embeds.shape[0], 0 if neg_embeds is None else neg_embeds.shape[0]
    if K != 64 or Df % 16 != 0:
        raise ValueError(f"{what}: K must be 64 and Df a multiple of 16")
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
    nbytes = int(lib.lsr_quick_query_plan_bytes(L, K, Df, n_pos, n_neg))
    if nbytes == 0:
        raise ValueError(f"{what}: unsupported shape")
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.lsr_quick_query_prepare(cb.data_ptr(), pos.data_ptr(), None if neg is None else neg.data_ptr(),
                                           L, K, Df, n_pos, n_neg, buf.data_ptr(), _stream(dev)),
               "lsr_quick_query_prepare")
    plan = QueryPlan(buf, L, K, Df, n_pos, n_neg)
    # the entry keeps the keyed tensors' storage (and their data_ptr) alive
    _PLANS[key] = (tensors, plan)
    while len(_PLANS) > _PLAN_CACHE_SIZE:
        _PLANS.popitem(last=False)
    return plan


def _chunks(pos_embeds: torch.Tensor, n_neg: int):
    """(q0, q1, pos_embeds[q0:q1]) over the positives, 64 - n_neg per kernel launch."""
    Q, step = pos_embeds.shape[0], _MAX_COLS - n_neg
    for q0 in range(0, Q, step):
        q1 = min(Q, q0 + step)
        yield q0, q1, pos_embeds if (q0, q1) == (0, Q) else pos_embeds[q0:q1]


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
    if mode == _lib.LSR_QUERY_RELEVANCY and not 1 <= n_neg < _MAX_COLS:
        raise ValueError(f"{what}: needs 1 to {_MAX_COLS - 1} negatives")
    if Q < 1:
        raise ValueError(f"{what}: needs at least one positive")
    if not (weight_map.is_cuda and codebooks.is_cuda):
        raise RuntimeError(f"{what}: tensors must be on the ROCm device (there is no CPU path)")
    hwc = _is_pixel_major(weight_map)
    wm = weight_map.detach() if hwc else weight_map.detach().contiguous().float()
    if out is None:
        out = torch.empty((L, Q, H, W), dtype=torch.float32, device=weight_map.device)
    elif (tuple(out.shape) != (L, Q, H, W) or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != weight_map.device):
        raise ValueError(f"{what}: out must be a contiguous float32 ({L}, {Q}, {H}, {W}) tensor")
    lib = _lib.load()
    layout = _lib.LSR_LAYOUT_HWC if hwc else _lib.LSR_LAYOUT_CHW
    for q0, q1, pos in _chunks(pos_embeds, n_neg):
        plan = query_plan(codebooks, pos, neg_embeds)
        # a chunk of the positives is written to a map of its own and copied into its planes
        dst = out if (q0, q1) == (0, Q) else torch.empty((L, q1 - q0, H, W), dtype=torch.float32, device=out.device)
        _lib.check(lib.lsr_quick_query_run(wm.data_ptr(), layout, plan.buf.data_ptr(), L, K, q1 - q0, n_neg, H, W,
                                           mode, float(scale), float(eps), dst.data_ptr(), _stream(wm.device)),
                   "lsr_quick_query_run")
        if dst is not out:
            out[:, q0:q1].copy_(dst)
    return out


@torch.no_grad()
def relevancy_maps(weight_map: torch.Tensor, codebooks: torch.Tensor, pos_embeds: torch.Tensor,
                   neg_embeds: torch.Tensor, *, scale: float = 10.0, eps: float = 1e-10,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """weight_map (L*K, H, W) fp32 CUDA (either layout, as for
    decode_language_features), codebooks (L, 64, Df), pos_embeds (Q, Df),
    neg_embeds (N_neg, Df) -> relevancy (L, Q, H, W) fp32: the values of
    get_max_across_quick applied to decode_language_features(weight_map,
    codebooks).  The embeddings may have any float dtype (the reference's are
    fp16); they are cast to fp32 and used as given — the caller normalises
    them, as the reference does in set_positives.  More than 64 - N_neg
    positives run in chunks.  scale >= 0 (the reference's 10)."""
    if scale < 0:
        raise ValueError("relevancy_maps: scale must be >= 0")
    return _maps("relevancy_maps", _lib.LSR_QUERY_RELEVANCY, weight_map, codebooks, pos_embeds, neg_embeds, scale,
                 eps, out)


@torch.no_grad()
def similarity_maps(weight_map: torch.Tensor, codebooks: torch.Tensor, embeds: torch.Tensor, *, eps: float = 1e-10,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-level cosine similarity (L, Q, H, W) of the normalised decoded
    feature f / (|f| + eps) with each of embeds (Q, Df)."""
    return _maps("similarity_maps", _lib.LSR_QUERY_COSINE, weight_map, codebooks, embeds, None, 0.0, eps, out)


class QuickRelevancyStream(_OverlapStream):
    """Render + relevancy over a stream of views, as quick.QuickFeatureStream
    does for the decode (the same push / flush contract and stream plumbing):
    the relevancy kernel of frame i runs on a side stream while frame i + 1
    renders; push returns the previous view's (L, Q, H, W) relevancy maps.
    Each frame's values equal relevancy_maps(weight map, ...) exactly."""

    def __init__(self, codebooks: torch.Tensor, pos_embeds: torch.Tensor, neg_embeds: torch.Tensor, *,
                 scale: float = 10.0, eps: float = 1e-10):
        super().__init__(codebooks.device)
        self.codebooks, self.pos_embeds, self.neg_embeds = codebooks, pos_embeds, neg_embeds
        self.scale, self.eps = float(scale), float(eps)
        # prepared on the caller's stream, which every later side-stream use is ordered after
        for _, _, pos in _chunks(pos_embeds, neg_embeds.shape[0]):
            query_plan(codebooks, pos, neg_embeds)

    def _alloc(self, wm):
        return torch.empty((self.codebooks.shape[0], self.pos_embeds.shape[0]) + tuple(wm.shape[1:]),
                           dtype=torch.float32, device=wm.device)

    def _run(self, wm, out):
        relevancy_maps(wm, self.codebooks, self.pos_embeds, self.neg_embeds, scale=self.scale, eps=self.eps, out=out)
