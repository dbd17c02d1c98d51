"""Generate tests/golden/ref_lang_l1.npz: the feature-phase loss under
--l1_loss, --l1_loss --normalize and --cos_loss --l1_loss --normalize, with
its autograd gradients, computed with the REFERENCE's own l1_loss and
cos_loss (utils/loss_utils.py:18-25, imported from the reference checkout on
the CPU) in float64.

The steps around them follow the reference's lines (restated here, since
scene.* does not import without plyfile/cv2, and compute_layer_feature_map
hard-codes 512 channels):
  f = codebooks[0].T @ weight_map.view(K, -1)             scene/gaussian_model.py:533-543 (layer 0)
  if --normalize: f = f / (f.norm(dim=0, keepdim=True) + 1e-10)          train.py:157-158
  gt = feature_map[seg].permute, mask = seg != -1         scene/cameras.py:77-94
  loss = [cos_loss(f*mask, gt*mask)] + l1_loss(f*mask, gt*mask)          train.py:159-167

Two cases: a (Df = 512, 6 x 9 pixels) and b (Df = 128, 12 x 20 pixels).  The
weight columns are top-4 sparse, as the rasterizer's are; case a uses 8 of
the 64 codes (the others' codebook gradient rows are exactly zero), case b
all of them, with a third of its pixels masked.  Each case has a fully masked
pixel and an all-zero weight column inside a segment (|f| = 0: the --normalize
subgradient).  The expected values are computed from the float32-rounded
inputs, in float64.
Run:  python tests/golden/make_ref_lang_l1.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("LSR_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
from utils.loss_utils import cos_loss, l1_loss  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_lang_l1.npz")
CONFIGS = {"l1": (False, False), "l1n": (True, False), "cl1n": (True, True)}   # name: (normalize, cos)


def case(g, K, Df, H, W, S, codes_used, masked):
    P = H * W
    wm = torch.zeros(K, P, dtype=torch.float64)
    for p in range(P):
        idx = torch.randperm(codes_used, generator=g)[:4]
        wm[idx, p] = torch.softmax(torch.randn(4, generator=g, dtype=torch.float64), 0) * torch.rand(
            1, generator=g, dtype=torch.float64)
    wm = wm.reshape(K, H, W)
    wm[:, 0, 1] = 0.0                                       # |f| = 0 inside a segment
    cb = torch.randn(1, K, Df, generator=g, dtype=torch.float64)
    feat = torch.randn(S, Df, generator=g, dtype=torch.float64)
    feat = feat / feat.norm(dim=1, keepdim=True)            # CLIP rows are unit vectors
    seg = torch.randint(0, S, (H, W), generator=g)
    seg[torch.rand(H, W, generator=g) < masked] = -1
    seg[0, 1] = 0
    seg[0, 2] = -1                                          # a fully masked pixel
    return wm, cb, seg, feat


def reference_loss(wm, cb, seg, feat, normalize, cos):
    K, H, W = wm.shape
    f = (cb[0].T @ wm.reshape(K, -1)).reshape(-1, H, W)
    if normalize:
        f = f / (f.norm(dim=0, keepdim=True) + 1e-10)
    s = seg.reshape(-1)
    mask = (s != -1).reshape(1, H, W)
    gt = feat[s].reshape(H, W, -1).permute(2, 0, 1)
    loss = 0
    if cos:
        loss = loss + cos_loss(f * mask, gt * mask)
    return loss + l1_loss(f * mask, gt * mask)


def main():
    g = torch.Generator().manual_seed(2025)
    out = {}
    for name, (Df, H, W, S, used, masked) in {"a": (512, 6, 9, 5, 8, 0.1), "b": (128, 12, 20, 7, 64, 0.33)}.items():
        wm, cb, seg, feat = case(g, 64, Df, H, W, S, used, masked)
        out[f"{name}_weight_map"] = wm.float().numpy()
        out[f"{name}_codebooks"] = cb.float().numpy()
        out[f"{name}_seg"] = seg.numpy().astype(np.int32)
        out[f"{name}_features"] = feat.float().numpy()
        for cfg, (normalize, cos) in CONFIGS.items():
            wm32 = torch.from_numpy(out[f"{name}_weight_map"]).double().requires_grad_(True)
            cb32 = torch.from_numpy(out[f"{name}_codebooks"]).double().requires_grad_(True)
            loss = reference_loss(wm32, cb32, seg, torch.from_numpy(out[f"{name}_features"]).double(), normalize, cos)
            loss.backward()
            out[f"{name}_{cfg}_loss"] = np.float64(loss.item())
            out[f"{name}_{cfg}_grad_weight_map"] = wm32.grad.numpy()
            out[f"{name}_{cfg}_grad_codebooks"] = cb32.grad.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
