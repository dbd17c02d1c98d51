"""Generate tests/golden/ref_relevancy.npz by running the REFERENCE's own
OpenCLIPNetwork.get_max_across_quick (eval/openclip_encoder.py:114-139) on a
seeded quick weight map, on the CPU.

The reference module imports open_clip and torchvision at its top; neither is
needed by get_max_across_quick, so empty stub modules stand in for them (for
generation only).  The method is called unbound on a SimpleNamespace carrying
the four attributes it reads (positives, negatives, pos_embeds, neg_embeds).
The semantic map it is given is built by the reference's post-render lines
(eval_lerf.py:214-218: einsum over the codebooks, then / (norm + 1e-10)) in
float64 — the reference function is dtype-generic — so the stored output is the
float64 value of the reference's formula; the reference's own fp32 result's
deviation from it is recorded too (ref_fp32_max_dev).

Run:  python tests/golden/make_ref_relevancy.py   (needs the reference tree,
LSR_REFERENCE or /root/reference; only the .npz is committed).
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

REF = os.environ.get("LSR_REFERENCE", "/root/reference")
for name in ("open_clip", "torchvision"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.path.insert(0, REF)
from eval.openclip_encoder import OpenCLIPNetwork  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_relevancy.npz")


def semantic_map(wmap, cb, dtype):
    """eval_lerf.py:214-218, then the (L, H, W, Df) permutation of its callers."""
    L, K, Df = cb.shape
    D, H, W = wmap.shape
    w = torch.from_numpy(wmap).to(dtype).view(L, K, H, W).view(L, K, H * W)
    c = torch.from_numpy(cb).to(dtype).permute(0, 2, 1)
    f = torch.einsum("ldk,lkn->ldn", c, w).view(L, Df, H, W)
    f = f / (f.norm(dim=1, keepdim=True) + 1e-10)
    return f.permute(0, 2, 3, 1)


def main():
    g = np.random.default_rng(20240611)
    L, K, Df, H, W, Q, N = 3, 64, 512, 12, 20, 3, 4
    wmap = (g.random((L * K, H, W)) * (g.random((L * K, H, W)) < 0.15)).astype(np.float32)
    wmap[:, 2, 3] = 0.0                                                   # an all-zero pixel
    wmap[:, 7, 11] = (wmap[:, 7, 11].astype(np.float64) * 1e-12).astype(np.float32)   # |f| comparable to eps
    cb = g.standard_normal((L, K, Df)).astype(np.float32)
    pos = g.standard_normal((Q, Df))
    neg = g.standard_normal((N, Df))
    pos = (pos / np.linalg.norm(pos, axis=1, keepdims=True)).astype(np.float32)
    neg = (neg / np.linalg.norm(neg, axis=1, keepdims=True)).astype(np.float32)

    def run(dtype):
        ns = SimpleNamespace(positives=("p",) * Q, negatives=("n",) * N, pos_embeds=torch.from_numpy(pos),
                             neg_embeds=torch.from_numpy(neg))
        with torch.no_grad():
            return OpenCLIPNetwork.get_max_across_quick(ns, semantic_map(wmap, cb, dtype)).double().numpy()

    r64, r32 = run(torch.float64), run(torch.float32)
    assert r64.shape == (L, Q, H, W)
    dev = float(np.abs(r32 - r64).max())
    np.savez_compressed(OUT, weight_map=wmap, codebooks=cb, pos_embeds=pos, neg_embeds=neg, relevancy=r64,
                        ref_fp32_max_dev=np.float64(dev), zero_pixel=np.array([2, 3]), tiny_pixel=np.array([7, 11]))
    print("wrote", OUT, os.path.getsize(OUT), "bytes; reference fp32 vs float64 max deviation", dev)


if __name__ == "__main__":
    main()
