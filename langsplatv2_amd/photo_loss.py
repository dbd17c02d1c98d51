"""Photometric loss of the RGB training step, fused on the GPU.

The reference's per-iteration loss after render() (train.py:170-173):

    Ll1 = l1_loss(image, gt_image)                                      utils/loss_utils.py:18-19
    loss = (1.0 - opt.lambda_dssim) * Ll1 + opt.lambda_dssim * (1.0 - ssim(image, gt_image))
        # ssim: five depthwise 11x11 conv2d calls + ~15 elementwise passes   utils/loss_utils.py:41-71

`photometric_loss` computes the same loss and its gradient w.r.t. the image
with one HIP pass per direction (csrc/photo_loss.hip, C ABI
lsr_photo_loss_forward/backward): the forward leaves both means and three
per-pixel derivative maps, the backward gathers the image gradient from them
(no atomics).  The two means are bit-identical from run to run.  `ssim` and
`l1_loss` have the reference's signatures, so
`from langsplatv2_amd.photo_loss import l1_loss, ssim` replaces
`from utils.loss_utils import l1_loss, ssim`.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib
from .rasterizer import _Alloc, _stream


def _args(image, gt, who):
    if image.dim() not in (3, 4):
        raise ValueError(f"{who}: image must be (C, H, W) or (B, C, H, W), got {tuple(image.shape)}")
    if tuple(image.shape) != tuple(gt.shape):
        raise ValueError(f"{who}: image {tuple(image.shape)} and gt {tuple(gt.shape)} differ in shape")
    for t, n in ((image, "image"), (gt, "gt")):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {n} must be a ROCm device tensor (there is no CPU path)")
    if image.numel() == 0:
        raise ValueError(f"{who}: empty image {tuple(image.shape)}")
    H, W = image.shape[-2:]
    return image.detach().contiguous().float(), gt.detach().contiguous().float(), image.numel() // (H * W), H, W


class _L1SSIM(torch.autograd.Function):
    """(mean |image - gt|, mean SSIM) as two 0-d tensors; the gradient goes to image only."""

    @staticmethod
    def forward(ctx, image, gt, with_partials=None):
        x, y, planes, H, W = _args(image, gt, "photometric_loss")
        out = torch.empty((2,), dtype=torch.float32, device=x.device)
        # grad mode is off in here, so the callers below pass whether a backward can follow
        if with_partials is None:
            with_partials = ctx.needs_input_grad[0]
        partials = torch.empty((3,) + tuple(x.shape), dtype=torch.float32, device=x.device) if with_partials else None
        alloc = _Alloc(x.device)
        _lib.check(_lib.load().lsr_photo_loss_forward(x.data_ptr(), y.data_ptr(), planes, H, W, out.data_ptr(),
                                                      partials.data_ptr() if partials is not None else None,
                                                      alloc.fn, None, _stream(x.device)), "lsr_photo_loss_forward")
        if partials is not None:
            ctx.save_for_backward(x, y, partials)
        ctx.dims = (planes, H, W)
        ctx.in_dtype = image.dtype
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        if not ctx.saved_tensors:   # the image took no gradient
            return None, None, None
        x, y, partials = ctx.saved_tensors
        planes, H, W = ctx.dims
        g = torch.stack((g_l1.detach().reshape(()), g_ssim.detach().reshape(()))).float().contiguous()
        gx = torch.empty_like(x)
        _lib.check(_lib.load().lsr_photo_loss_backward(x.data_ptr(), y.data_ptr(), planes, H, W,
                                                       partials.data_ptr(), g.data_ptr(), gx.data_ptr(),
                                                       _stream(x.device)), "lsr_photo_loss_backward")
        return gx.to(ctx.in_dtype), None, None


def _apply(image, gt):
    return _L1SSIM.apply(image, gt, bool(torch.is_grad_enabled() and image.requires_grad))


def l1_ssim(image: torch.Tensor, gt: torch.Tensor) -> tuple:
    """(Ll1, ssim) of train.py:170-171 from one fused forward: image and gt
    (C, H, W) or (B, C, H, W) device tensors of equal shape.  Differentiable
    w.r.t. image."""
    return _apply(image, gt)


def photometric_loss(image: torch.Tensor, gt: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)): train.py:171-172."""
    l1, s = _apply(image, gt)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s)


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """utils/loss_utils.py:41-49 (mean SSIM, 11x11 Gaussian window, sigma 1.5); the
    only window the kernel is built for is the reference's default."""
    if window_size != 11:
        raise ValueError(f"ssim: window_size={window_size} (the fused kernel has the reference's 11-tap window only)")
    if not size_average:
        raise ValueError("ssim: size_average=False is not supported (the fused kernel returns the mean)")
    return _apply(img1, img2)[1]


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """utils/loss_utils.py:18-19 (the same fused pass, its SSIM output unused)."""
    return _apply(network_output, gt)[0]


__all__ = ["photometric_loss", "l1_ssim", "ssim", "l1_loss"]
