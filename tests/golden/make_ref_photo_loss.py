"""Generate tests/golden/ref_photo_loss.npz by running the REFERENCE's own loss
utilities (utils/loss_utils.py:18-71: l1_loss, ssim) in float64 under autograd,
as train.py:170-172 combines them (lambda_dssim = 0.2), on seeded images.
Pins langsplatv2_amd/photo_loss.py (tests/test_photo_loss.py).

The inputs are generated in fp32 and those exact values are upcast for the
float64 run: a reference made from unrounded doubles flips sign(x - y) where
the noise is below one fp32 ulp.

Run:  LSR_REFERENCE=<reference checkout> python tests/golden/make_ref_photo_loss.py
(only the resulting .npz is committed and travels)."""
import os
import sys

import numpy as np
import torch

if not os.environ.get("LSR_REFERENCE"):
    sys.exit("set LSR_REFERENCE to the reference checkout (the directory holding utils/loss_utils.py)")
sys.path.insert(0, os.environ["LSR_REFERENCE"])
from utils import loss_utils  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_photo_loss.npz")
LAMBDA = 0.2
# name -> (shape, kind): the shapes of tests/test_photo_loss.py (the kernel's tile is 64 x 16)
CASES = {
    "noisy_3x11x17": ((3, 11, 17), "noisy"),          # as ref_ssim.npz
    "noisy_1x5x3": ((1, 5, 3), "noisy"),              # smaller than the window: every tap is padding somewhere
    "smooth_3x33x65": ((3, 33, 65), "smooth"),        # one pixel past a 16/32/64 tile multiple in both dimensions
    "smooth_3x64x128": ((3, 64, 128), "smooth"),      # exact tile multiples
    "smooth_2x3x24x40": ((2, 3, 24, 40), "smooth"),   # batched
}


def noisy(shape, g):
    y = torch.rand(shape, generator=g)
    x = (y + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    return x, y


def smooth(shape, g):
    """The regime of real renders (small D, fp32 cancellation in e11 - mu1^2
    amplified), with x = y exactly on the top-left H/2 x W/3 patch (sign(0), m = 1)."""
    H, W = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    c = torch.arange(planes, dtype=torch.float32).view(planes, 1, 1)
    y = (0.5 + 0.4 * torch.sin(xx / 9 + c) * torch.cos(yy / 7)).reshape(shape)
    x = (y + 0.02 * torch.randn(shape, generator=g)).clamp(0, 1)
    x[..., :H // 2, :W // 3] = y[..., :H // 2, :W // 3]
    return x, y


def main():
    g = torch.Generator().manual_seed(11)
    out = {}
    for name, (shape, kind) in CASES.items():
        x, y = (noisy if kind == "noisy" else smooth)(shape, g)
        x, y = x.float().contiguous(), y.float().contiguous()
        xd = x.double().requires_grad_(True)
        yd = y.double()
        l1 = loss_utils.l1_loss(xd, yd)
        ss = loss_utils.ssim(xd, yd)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ss)
        loss.backward()
        out[f"{name}_x"] = x.numpy()
        out[f"{name}_y"] = y.numpy()
        out[f"{name}_l1"] = np.float64(l1.item())
        out[f"{name}_ssim"] = np.float64(ss.item())
        out[f"{name}_loss"] = np.float64(loss.item())
        out[f"{name}_grad"] = xd.grad.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
