"""RGB-phase photometric loss at one training view: the fused HIP pair
(langsplatv2_amd.photo_loss.photometric_loss) vs the torch formulation it replaces
(train_loop.view_loss: five depthwise 11x11 conv2d + elementwise passes, autograd in
reverse) on the same GPU, forward + backward, seeded smooth pattern plus noise.

  python tools/bench_photo_loss.py [--iters 200] [--out profiles/photo_loss_bench.json]
Prints one JSON line per variant and size (ms per loss fwd+bwd, algorithmic bytes).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from langsplatv2_amd.photo_loss import photometric_loss  # noqa: E402
from langsplatv2_amd.train_loop import view_loss  # noqa: E402

SIZES = ((3, 800, 1280), (3, 1080, 1920))
LAMBDA = 0.2
# per pixel (three channels): x and y read twice (24 + 24 B), three partial maps written
# and read (36 + 36 B), the gradient written (12 B)
BYTES_PER_PIXEL = 132


def images(shape, dev):
    C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    c = torch.arange(C, device=dev, dtype=torch.float32).view(C, 1, 1)
    gt = 0.5 + 0.4 * torch.sin(xx / 9 + c) * torch.cos(yy / 7)
    img = (gt + 0.02 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    return img.requires_grad_(True), gt


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for shape in SIZES:
        img, gt = images(shape, dev)

        def run(loss_fn):
            img.grad = None
            loss_fn(img, gt, LAMBDA).backward()

        alg = BYTES_PER_PIXEL * shape[1] * shape[2]
        # alternate the two variants so a busy neighbour hits both alike
        ms_f, ms_t = [], []
        for _ in range(3):
            ms_f.append(timed(lambda: run(photometric_loss), a.iters))
            ms_t.append(timed(lambda: run(view_loss), a.iters))
        f, t = min(ms_f), min(ms_t)
        with torch.no_grad():
            l_f, l_t = photometric_loss(img, gt, LAMBDA).item(), view_loss(img, gt, LAMBDA).item()
        lines.append({"variant": "fused_hip", "C": shape[0], "H": shape[1], "W": shape[2], "ms_fwd_bwd": round(f, 4),
                      "ms_runs": [round(v, 4) for v in ms_f], "algorithmic_bytes": alg,
                      "GBps": round(alg / f / 1e6, 1), "loss": l_f})
        lines.append({"variant": "torch_view_loss", "C": shape[0], "H": shape[1], "W": shape[2],
                      "ms_fwd_bwd": round(t, 4), "ms_runs": [round(v, 4) for v in ms_t],
                      "speedup_fused": round(t / f, 2), "loss": l_t})
        for ln in lines[-2:]:
            print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(ln) for ln in lines) + "\n")


if __name__ == "__main__":
    main()
